"""Knob 85: CG mode 5's fused direction + p.Ap pass (spmv_pair_pbw_kernel,
knob 69) with the workgroup's four waves passing each plane's centre p_i
through LDS instead of forming the +n line's and the +1 edge's p_i again from
their own loads of r and p_{i-1}.  Every wave keeps its units, its row sums
and its partial sums, and the owner formed the passed values with the same
expression from the same operands, so the whole solve -- its, reason, residual
history, x -- is bitwise the unshared kernel's; the dispatch count `zm_shared`
shows which form ran.

(The same exchange in the two-line residual update, spmv_pair_zm2l_kernel,
was built and measured slower at every size -- DESIGN.md section 13 -- and is
not in the tree: the residual update here is the unshared one in both runs,
forced to the two-line form by knob 68 = 2.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nx, ny, nz) that take the shared form; see test_shared_fused_pass_bitwise's
# docstring for the cases and the substitutions
SHARED = [
    (128, 8, 9),      # lines of one unit: four lines per group, every +n but the group's last line's, no edges
    (256, 8, 17),     # lines of two units (the 256^3 geometry)                       [for (256, 4, 17)]
    (512, 8, 9),      # lines of four units: edge sharing only, wave 3 at the line end [for (512, 2, 5)]
    (256, 16, 6),     # fewer planes than XCDs: some XCDs have no task                [for (256, 8, 3)]
    (256, 6, 9),      # 12 columns per plane: three groups of two lines (an odd number of groups)
    (1024, 8, 9),     # lines of eight units: wave 3 of a line's first group takes its +1 edge from outside the workgroup
    (256, 128, 40),   # segments of 3 planes with a 2-plane last one: the two-plane step, its one-plane tail, buffers reused
    (128, 128, 128),  # segments of 4 planes: two two-plane steps per task, every buffer used twice
]
# the host declines: 14 columns per plane (not a multiple of 4), and lines of
# three units (a group of four columns would straddle lines unevenly)
FALLBACK = [(256, 7, 9), (384, 8, 9)]


def _solve_pair(comm, dims, pc="jacobi", guess=False, max_it=10000):
    """The same solve with knob 85 off, then on: (its, reason, history, x, cg_mode, dispatch) each."""
    from mxsolve import _lib
    from mxsolve.core import DMat, dispatch_counts, rhs_hash
    L = _lib.load()
    old27 = L.mx_debug_set(27, 1)
    try:
        A = DMat.stencil(comm, "poisson3d", *dims)
    finally:
        L.mx_debug_set(27, old27)
    m = A.info()["m"]
    b = comm.empty(m)
    rhs_hash(comm, 0, b)
    x0 = None
    if guess:
        x0 = comm.empty(m)
        rhs_hash(comm, 5, x0)
        x0.mul_(1e-3)
    outs = []
    for k85 in (0, 1):
        old = {k: L.mx_debug_set(k, v) for k, v in ((9, 5), (27, 1), (68, 2), (69, 1), (85, k85))}
        try:
            x = x0.clone() if guess else comm.zeros(m)
            dispatch_counts(reset=True)
            r = A.solve(b, x, ksp="cg", pc=pc, rtol=1e-8, max_it=max_it, history=True, guess_nonzero=guess)
            dc = dispatch_counts(reset=True)
            outs.append((r["its"], r["reason"], r["history"].copy(), x.cpu().numpy().copy(), r["cg_mode"], dc))
        finally:
            for k, v in old.items():
                L.mx_debug_set(k, v)
    A.destroy()
    return outs


def _assert_bitwise(a, c):
    assert a[4] == c[4] == 5, (a[4], c[4])
    for k in ("zm_pbw", "zm_pw", "zm_rupd"):
        assert a[5][k] > 0 and c[5][k] == a[5][k], (a[5], c[5])
    assert a[:2] == c[:2], (a[:2], c[:2])
    assert a[0] > 0
    assert np.array_equal(a[2].view(np.uint64), c[2].view(np.uint64))
    assert np.array_equal(a[3].view(np.uint64), c[3].view(np.uint64))


@pytest.mark.parametrize("dims,pc,guess,max_it", [
    (SHARED[0], "jacobi", False, 10000),
    (SHARED[0], "none", False, 10000),
    (SHARED[1], "jacobi", False, 10000),
    (SHARED[1], "none", True, 10000),
    (SHARED[1], "jacobi", False, 7),
    (SHARED[2], "jacobi", False, 10000),
    (SHARED[2], "none", False, 10000),
    (SHARED[3], "jacobi", True, 10000),
    (SHARED[4], "jacobi", False, 10000),
    (SHARED[5], "jacobi", False, 10000),
    (SHARED[6], "jacobi", False, 10000),
    (SHARED[6], "none", True, 37),
    (SHARED[7], "jacobi", False, 10000),
])
def test_shared_fused_pass_bitwise(selfcomm, dims, pc, guess, max_it):
    """The shared form runs (zm_shared counts once per fused-pass launch, beside
    zm_pbw) and the solve is bit for bit the unshared one's: Jacobi and no
    preconditioner, a nonzero guess, and a max_it that stops inside an x-step
    batch.

    Substitutions.  The row-pair layout -- and with it CG mode 5 -- needs more
    than half the rows interior, so the issue's (256, 4, 17), (512, 2, 5) and
    (256, 8, 3) run mode 2 on the general kernel (dispatch: only `sell`); each
    is replaced by the nearest shape of the same neighbour case that reaches
    the z-march kernels: (256, 8, 17), (512, 8, 9), (256, 16, 6).  Its
    fallback shapes do not serve the fused pass, which has one line per wave:
    (256, 6, 9) has 12 columns per plane and shares (it is in SHARED), and
    (256, 2, 9) does not reach mode 5; (256, 7, 9) and (384, 8, 9) are the
    declined shapes.  The small shapes have so few columns that the z-march
    gives every task one plane; (256, 128, 40) and 128^3 have segments of 3
    (the last of 2) and 4 planes, so they run the two-plane step with its
    second exchange, the one-plane tail and the reuse of both buffers."""
    a, c = _solve_pair(selfcomm, dims, pc, guess, max_it)
    _assert_bitwise(a, c)
    assert a[5]["zm_shared"] == 0, a[5]
    assert c[5]["zm_shared"] == c[5]["zm_pbw"], c[5]


@pytest.mark.parametrize("dims", FALLBACK)
def test_shared_declined_runs_unshared(selfcomm, dims):
    """A workgroup's waves would not hold one aligned group of whole lines (or
    units of one line) of one segment, so the host keeps the unshared kernel --
    zm_shared stays 0 and the solve is the same bits."""
    a, c = _solve_pair(selfcomm, dims)
    _assert_bitwise(a, c)
    assert a[5]["zm_shared"] == 0 and c[5]["zm_shared"] == 0, (a[5], c[5])
