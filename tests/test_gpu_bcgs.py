"""BiCGStab (KSPBCGS, mx_bcgs.hpp) on the GPU against its numpy restatement
(tests/_bcgs_ref.py with np.dot; the inputs' margins are checked in
test_cpu_bcgs.py).  Bar, the project's for CG / GMRES: its and reason equal,
x within relative L2 1e-10, the residual history its + 1 entries long and
each within relative 1e-8.

Solves run to convergence are compared on the systems whose iterates do not
hang on the summation order (_bcgs_ref.CONVERGED); the convection-diffusion
stencil at 16^3 and 24 x 20 x 12 does (_bcgs_ref.py has the figures), so those
two are compared over their first 12 iterations."""
import numpy as np
import pytest
import torch

import _bcgs_ref as ref

pytestmark = pytest.mark.gpu
REL_TOL = 1e-10
HIST_TOL = 1e-8


def _knob(k, v):
    from mxsolve import _lib
    return _lib.load().mx_debug_set(k, v)


def _mat(comm, ip, c, v, cb=None):
    from mxsolve.core import DMat
    M = ip.size - 1
    if cb is None:
        return DMat.from_csr(comm, M, M, ip, c, v)
    old = _knob(84, cb)
    try:
        return DMat.from_csr(comm, M, M, ip, c, v)
    finally:
        _knob(84, old)


def _solve(A, b, x0=None, **kw):
    """One device solve; returns (result dict, x as numpy)."""
    bt = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    xt = torch.zeros_like(bt) if x0 is None else torch.from_numpy(np.ascontiguousarray(x0)).cuda()
    r = A.solve(bt, xt, ksp="bcgs", history=True, guess_nonzero=x0 is not None, **kw)
    return r, xt.cpu().numpy()


def _check(r, x, o):
    if r["history"].size == o["history"].size:
        print("its", r["its"], "reason", r["reason"], "x rel-L2", np.linalg.norm(x - o["x"]) / np.linalg.norm(o["x"]),
              "history rel", np.max(np.abs(r["history"] - o["history"]) / np.abs(o["history"])))
    assert (r["its"], r["reason"]) == (o["its"], o["reason"]), (r["its"], r["reason"], o["its"], o["reason"])
    assert np.linalg.norm(x - o["x"]) <= REL_TOL * np.linalg.norm(o["x"])
    assert r["history"].size == r["its"] + 1
    assert np.all(np.abs(r["history"] - o["history"]) <= HIST_TOL * np.abs(o["history"]))
    assert r["launched_its"] >= r["its"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def mats(selfcomm, oracle_mod):
    """The named systems' device operators, assembled once for the module."""
    made = {}

    def get(name):
        if name not in made:
            ip, c, v = ref.system(oracle_mod, name)[:3]
            made[name] = _mat(selfcomm, ip, c, v)
        return made[name]
    yield get
    for A in made.values():
        A.destroy()


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("name", ["convdiff8", "convdiff10", "convdiff13x10x9"])
def test_parity_stencils(mats, oracle_mod, name, pc):
    """8^3 (one workgroup), 10^3, 13 x 10 x 9 (1170 rows: odd line lengths, a
    tail in every 16-byte loop)."""
    b = ref.system(oracle_mod, name)[3]
    r, x = _solve(mats(name), b, pc=pc)
    _check(r, x, ref.reference(oracle_mod, name, pc))
    assert r["reason"] == 2


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("name", ref.TRUNCATED)
def test_parity_first_iterations_of_the_large_stencils(mats, oracle_mod, name, pc):
    b = ref.system(oracle_mod, name)[3]
    r, x = _solve(mats(name), b, pc=pc, max_it=ref.TRUNCATED_ITS)
    assert (r["its"], r["reason"]) == (ref.TRUNCATED_ITS, -3)
    _check(r, x, ref.reference(oracle_mod, name, pc, max_it=ref.TRUNCATED_ITS))


@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_parity_random_two_pass_and_one_pass(selfcomm, oracle_mod, pc):
    """N = 4099 (odd, no multiple of 64) x 7 nonsymmetric: once with the
    column-block two-pass MatMult (key 84 = 2), once with the one-pass SELL
    kernel (key 84 = 0) -- the same bits, and the reference's iterates."""
    from mxsolve.core import dispatch_counts
    ip, c, v, b, _ = ref.system(oracle_mod, "random4099")
    got = {}
    for cb in (2, 0):
        A = _mat(selfcomm, ip, c, v, cb)
        assert (A.info()["cb_blocks"] > 0) == (cb == 2)
        dispatch_counts(reset=True)
        got[cb] = _solve(A, b, pc=pc)
        dc = dispatch_counts(reset=True)
        assert (dc["cb"] >= 2 * got[cb][0]["its"]) == (cb == 2) and (dc["cb"] == 0) == (cb == 0)
        A.destroy()
    _check(*got[2], ref.reference(oracle_mod, "random4099", pc))
    assert np.array_equal(_bits(got[2][1]), _bits(got[0][1]))
    assert np.array_equal(_bits(got[2][0]["history"]), _bits(got[0][0]["history"]))


# ---------------------------------------------------------------- 2. which MatMult ran
def test_matmult_family_kernel_ran(mats, oracle_mod):
    from mxsolve.core import dispatch_counts
    b = ref.system(oracle_mod, "convdiff16")[3]
    dispatch_counts(reset=True)
    r, _ = _solve(mats("convdiff16"), b, pc="jacobi")
    dc = dispatch_counts(reset=True)
    assert max(dc.values()) >= 2 * r["its"] > 0, dc


# ---------------------------------------------------------------- 3. nonzero initial guess
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_nonzero_guess(mats, oracle_mod, pc):
    name = "convdiff13x10x9"
    O = ref.system(oracle_mod, name)[4]
    xt = ref.x_true(O.M)
    b = O.mult(xt)
    o = ref.bcgs_ref(O, b, pc=pc, x0=0.5 * xt)
    r, x = _solve(mats(name), b, x0=0.5 * xt, pc=pc)
    _check(r, x, o)
    assert r["its"] > 0 and r["reason"] == 2
    r, x = _solve(mats(name), b, x0=xt, pc=pc)
    assert r["its"] == 0 and r["reason"] > 0
    assert np.array_equal(_bits(x), _bits(xt))


# ---------------------------------------------------------------- 4. stopping rules
def test_max_it(mats, oracle_mod):
    b = ref.system(oracle_mod, "convdiff16")[3]
    r, x = _solve(mats("convdiff16"), b, pc="jacobi", max_it=3)
    assert (r["its"], r["reason"]) == (3, -3)
    _check(r, x, ref.reference(oracle_mod, "convdiff16", "jacobi", max_it=3))


def test_norm_none_and_unsupported_norm(mats, oracle_mod):
    from mxsolve._lib import MxError
    b = ref.system(oracle_mod, "convdiff16")[3]
    r, _ = _solve(mats("convdiff16"), b, pc="jacobi", max_it=5, norm="none")
    assert (r["its"], r["reason"]) == (5, 4)
    with pytest.raises(MxError, match="preconditioned norm only"):
        _solve(mats("convdiff16"), b, pc="jacobi", norm="unpreconditioned")
    with pytest.raises(MxError, match="preconditioned norm only"):
        _solve(mats("convdiff16"), b, pc="jacobi", norm="natural")


def test_zero_rhs(mats, oracle_mod):
    b = np.zeros(ref.system(oracle_mod, "convdiff16")[3].size)
    r, x = _solve(mats("convdiff16"), b, pc="jacobi")
    assert (r["its"], r["reason"]) == (0, 3) and not x.any()


def test_tight_rtol_true_residual(mats, oracle_mod):
    b, O = ref.system(oracle_mod, "convdiff16")[3:5]
    r, x = _solve(mats("convdiff16"), b, pc="jacobi", rtol=1e-10)
    assert r["reason"] == 2 and r["history"].size == r["its"] + 1
    assert r["history"][-1] <= 1e-10 * r["history"][0] < r["history"][-2]
    assert np.linalg.norm(b - O.mult(x)) <= 1e-8 * np.linalg.norm(b)


# ---------------------------------------------------------------- 5. breakdown, tiny systems
def test_breakdown_two_rows(selfcomm):
    A = _mat(selfcomm, np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([1.0, 1.0]))
    r, x = _solve(A, np.array([1.0, 0.0]), pc="none")
    A.destroy()
    assert (r["its"], r["reason"]) == (0, -5) and not x.any()
    assert r["history"].size == 1 and r["history"][0] == 1.0


@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_one_row(selfcomm, pc):
    A = _mat(selfcomm, np.array([0, 1], np.int64), np.array([0], np.int32), np.array([4.0]))
    r, x = _solve(A, np.array([2.0]), pc=pc)
    A.destroy()
    assert (r["its"], r["reason"]) == (1, 2) and x[0] == 0.5
    assert r["history"].size == 2 and r["history"][1] == 0.0


# ---------------------------------------------------------------- 6. polling and overrun
def test_poll_every(mats, oracle_mod):
    b = ref.system(oracle_mod, "convdiff13x10x9")[3]
    A = mats("convdiff13x10x9")
    r1, x1 = _solve(A, b, pc="jacobi", poll_every=1)
    r16, x16 = _solve(A, b, pc="jacobi", poll_every=16)
    assert r1["its"] == r16["its"] and r1["reason"] == r16["reason"]
    assert np.array_equal(_bits(x1), _bits(x16))
    assert np.array_equal(_bits(r1["history"]), _bits(r16["history"]))
    assert r1["launched_its"] >= r1["its"] and r16["launched_its"] >= r16["its"]
    assert r16["launched_its"] % 16 == 0 and r16["launched_its"] > r16["its"]   # iterations past the stop ran as no-ops


# ---------------------------------------------------------------- 7. determinism, uninitialised work space
def test_deterministic_and_poisoned_workspace(mats, oracle_mod):
    """Key 81 = 2: the buffer cache hands out blocks filled with 0xA5 bytes.
    The first iteration must read neither P nor V (P = R there)."""
    name = "convdiff24x20x12"
    b = ref.system(oracle_mod, name)[3]
    A = mats(name)
    r0, x0 = _solve(A, b, pc="jacobi")
    r1, x1 = _solve(A, b, pc="jacobi")
    assert np.array_equal(_bits(x0), _bits(x1)) and np.array_equal(_bits(r0["history"]), _bits(r1["history"]))
    old = _knob(81, 2)
    try:
        A.ksp_reset()
        r2, x2 = _solve(A, b, pc="jacobi")
    finally:
        _knob(81, old)
    assert r2["its"] == r0["its"] and r2["reason"] == r0["reason"]
    assert np.array_equal(_bits(x0), _bits(x2)) and np.array_equal(_bits(r0["history"]), _bits(r2["history"]))


def test_poisoned_workspace_large_enough_for_the_cache(selfcomm, oracle_mod):
    """The same with a work space above the cache's 1 MiB threshold (64^3: six
    2 MiB vectors), where a reused block really carries the fill."""
    from mxsolve.core import DMat, rhs_hash
    A = DMat.stencil(selfcomm, "convdiff3d", 64)
    M = A.info()["m"]
    b = selfcomm.empty(M)
    rhs_hash(selfcomm, 0, b)
    out = []
    old = _knob(81, 1)
    try:
        for poison in (1, 2):
            _knob(81, poison)
            A.ksp_reset()
            x = selfcomm.zeros(M)
            r = A.solve(b, x, ksp="bcgs", pc="jacobi", history=True)
            out.append((r["its"], r["reason"], r["history"], x.cpu().numpy()))
    finally:
        _knob(81, old)
        A.destroy()
    assert out[0][:2] == out[1][:2] and out[0][1] == 2
    assert np.array_equal(_bits(out[0][2]), _bits(out[1][2])) and np.array_equal(_bits(out[0][3]), _bits(out[1][3]))


# ---------------------------------------------------------------- 8. P > 1
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("name", ["convdiff13x10x9", "random4099"])
def test_ranks(mats, oracle_mod, name, P):
    from mxsolve.core import DMat, LocalWorld, layout_split
    ip, c, v, b, _ = ref.system(oracle_mod, name)
    M = ip.size - 1
    one, x_one = _solve(mats(name), b, pc="jacobi")
    ranges = layout_split(M, P)

    def body(comm):
        r0, r1 = int(ranges[comm.rank]), int(ranges[comm.rank + 1])
        A = DMat.from_csr(comm, M, M, ip[r0:r1 + 1] - ip[r0], c[ip[r0]:ip[r1]], v[ip[r0]:ip[r1]])
        bl = torch.from_numpy(b[r0:r1].copy()).cuda()
        xl = comm.zeros(r1 - r0)
        r = A.solve(bl, xl, ksp="bcgs", pc="jacobi", history=True)
        out = (r["its"], r["reason"], r["rnorm"], xl.cpu().numpy(), r["launched_its"])
        A.destroy()
        return out

    w = LocalWorld(P)
    try:
        res = w.run(body)
    finally:
        w.destroy()
    assert all(r[:3] == res[0][:3] for r in res), [r[:3] for r in res]
    assert all(r[4] == res[0][4] >= r[0] for r in res)
    assert (res[0][0], res[0][1]) == (one["its"], one["reason"])
    xs = np.concatenate([r[3] for r in res])
    assert np.linalg.norm(xs - x_one) <= REL_TOL * np.linalg.norm(x_one)


# ---------------------------------------------------------------- 9. the petsc4py shim
def _shim_solve(oracle_mod, configure):
    from mxsolve import PETSc
    ip, c, v, b, _ = ref.system(oracle_mod, "convdiff16")
    M = ip.size - 1
    A = PETSc.Mat().createAIJ(size=(M, M), csr=(ip, c, v))
    xv, bv = A.getVecs()
    bv.setArray(b)
    ksp = PETSc.KSP().create()
    ksp.setOperators(A)
    ksp.setConvergenceHistory()
    configure(PETSc, ksp)
    try:
        ksp.solve(bv, xv)
        return ksp, np.array(xv.array)
    finally:
        ksp.destroy()
        A.destroy()


def test_shim_set_type(oracle_mod, capsys):
    def configure(PETSc, ksp):
        ksp.setType(PETSc.KSP.Type.BCGS)
        assert PETSc.KSP.Type.BCGS == "bcgs"
        ksp.getPC().setType("jacobi")
    ksp, x = _shim_solve(oracle_mod, configure)
    o = ref.reference(oracle_mod, "convdiff16", "jacobi")
    assert ksp.getIterationNumber() == o["its"] and ksp.getConvergedReason() == 2
    h = ksp.getConvergenceHistory()
    assert h.size == o["its"] + 1 and ksp.getResidualNorm() == h[-1]
    assert np.all(np.abs(h[:8] - o["history"][:8]) <= HIST_TOL * o["history"][:8])
    ksp.view()
    assert "type: bcgs" in capsys.readouterr().out


def test_shim_options(oracle_mod, capsys):
    from mxsolve import PETSc
    opts = PETSc.Options()
    keys = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_monitor": None, "ksp_converged_reason": None}
    for k, val in keys.items():
        opts[k] = val
    try:
        ksp, _ = _shim_solve(oracle_mod, lambda P, k: k.setFromOptions())
    finally:
        for k in keys:
            opts.delValue(k)
    o = ref.reference(oracle_mod, "convdiff16", "jacobi")
    assert ksp.getType() == "bcgs"
    assert ksp.getIterationNumber() == o["its"] and ksp.getConvergedReason() == 2
    out = capsys.readouterr().out
    assert f"{o['its']:3d} KSP Residual norm" in out
    assert f"Linear solve converged due to CONVERGED_RTOL iterations {o['its']}" in out


@pytest.mark.parametrize("kt", ["fgmres", "richardson"])
def test_shim_unsupported_types_still_raise(oracle_mod, kt):
    from mxsolve import PETSc
    with pytest.raises(PETSc.Error, match="bcgs"):
        _shim_solve(oracle_mod, lambda P, k: k.setType(kt))
