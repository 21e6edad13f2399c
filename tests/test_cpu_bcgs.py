"""BiCGStab without a GPU: the ABI value, and the conditions the GPU tests'
inputs must meet so that `its` is a property of the system, not of a
summation order -- the numpy restatement (tests/_bcgs_ref.py) run with three
dot-product orders agrees on its / reason, its x agree to 1e-12, and the
stopping residual clears the threshold by a margin (last entry <= 0.99 ttol,
the one before >= 1.01 ttol).

The library's convection-diffusion stencil does not meet them at 16^3 and
24 x 20 x 12 run to convergence (figures in _bcgs_ref.py, printed by
test_recorded_sensitivity_of_the_large_stencils): those shapes are compared
over their first 12 iterations, where the orders agree to 1e-12."""
import os
import re

import numpy as np
import pytest

import _bcgs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_value():
    from mxsolve import core
    assert core.KSP_TYPES["bcgs"] == 3
    hdr = open(os.path.join(ROOT, "include", "mxsolve.h")).read()
    assert re.search(r"\bMX_KSP_BCGS\s*=\s*3\b", hdr)
    assert re.search(r"#define\s+MX_ABI_VERSION\s+3\b", hdr)


def _three_orders(O, b, pc, **kw):
    runs = {k: ref.bcgs_ref(O, b, pc=pc, dot=d, **kw) for k, d in ref.DOTS.items()}
    base = runs["np.dot"]
    hd = max(np.max(np.abs(r["history"] - base["history"]) / base["history"]) for r in runs.values())
    xd = max(np.linalg.norm(r["x"] - base["x"]) for r in runs.values()) / np.linalg.norm(base["x"])
    print("its", [r["its"] for r in runs.values()], "reason", base["reason"], "history rel", hd, "x rel-L2", xd,
          "last/ttol", base["history"][-1] / base["ttol"], "previous/ttol", base["history"][-2] / base["ttol"])
    return runs, base, hd, xd


def _agree(runs, base):
    for k, r in runs.items():
        assert (r["its"], r["reason"]) == (base["its"], base["reason"]), k
        assert np.linalg.norm(r["x"] - base["x"]) <= 1e-12 * np.linalg.norm(base["x"]), k
        assert r["history"].size == r["its"] + 1


def _margins(runs):
    for k, r in runs.items():
        assert r["history"][-1] <= 0.99 * r["ttol"], k
        assert r["history"][-2] >= 1.01 * r["ttol"], k


# every matrix / PC case test_gpu_bcgs.py runs to convergence against the reference
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("name", ref.CONVERGED)
def test_converged_cases_well_conditioned(oracle_mod, name, pc):
    ip, c, v, b, O = ref.system(oracle_mod, name)
    runs, base, _, _ = _three_orders(O, b, pc)
    assert base["reason"] == ref.RTOL and base["its"] >= 2
    _agree(runs, base)
    _margins(runs)


@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_nonzero_guess_case_well_conditioned(oracle_mod, pc):
    O = ref.system(oracle_mod, "convdiff13x10x9")[4]
    xt = ref.x_true(O.M)
    runs, base, _, _ = _three_orders(O, O.mult(xt), pc, x0=0.5 * xt)
    assert base["reason"] == ref.RTOL and base["its"] >= 2
    _agree(runs, base)
    _margins(runs)


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("name", ref.TRUNCATED)
def test_truncated_cases_well_conditioned(oracle_mod, name, pc):
    ip, c, v, b, O = ref.system(oracle_mod, name)
    runs, base, hd, _ = _three_orders(O, b, pc, max_it=ref.TRUNCATED_ITS)
    assert (base["its"], base["reason"]) == (ref.TRUNCATED_ITS, ref.DIV_ITS)
    _agree(runs, base)
    assert hd <= 1e-10


def test_its_of_the_16_cubed_case_does_not_hang_on_the_order(oracle_mod):
    """The shim tests compare only its / reason on 16^3 + Jacobi: the three
    orders agree on them, with the margins."""
    ip, c, v, b, O = ref.system(oracle_mod, "convdiff16")
    runs, base, _, _ = _three_orders(O, b, "jacobi")
    assert all((r["its"], r["reason"]) == (base["its"], ref.RTOL) for r in runs.values())
    _margins(runs)


@pytest.mark.parametrize("name", ref.TRUNCATED)
def test_recorded_sensitivity_of_the_large_stencils(oracle_mod, name):
    """Recorded, not gated: what the summation order does to these shapes
    when run to convergence (why they are not parity cases)."""
    ip, c, v, b, O = ref.system(oracle_mod, name)
    for pc in ("jacobi", "none"):
        _three_orders(O, b, pc)


def test_breakdown_and_one_row(oracle_mod):
    O = oracle_mod.OracleMat.from_csr(2, 2, np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, 1.0]))
    r = ref.bcgs_ref(O, np.array([1.0, 0.0]), pc="none")
    assert (r["its"], r["reason"]) == (0, ref.BREAKDOWN) and not r["x"].any()
    O = oracle_mod.OracleMat.from_csr(1, 1, np.array([0, 1]), np.array([0]), np.array([4.0]))
    for pc in ("none", "jacobi"):
        r = ref.bcgs_ref(O, np.array([2.0]), pc=pc)
        assert (r["its"], r["reason"]) == (1, ref.RTOL) and r["x"][0] == 0.5


def test_stopping_rules_of_the_reference(oracle_mod):
    ip, c, v, b, O = ref.system(oracle_mod, "convdiff16")
    r = ref.bcgs_ref(O, b, max_it=3)
    assert (r["its"], r["reason"]) == (3, ref.DIV_ITS)
    r = ref.bcgs_ref(O, b, max_it=5, norm="none")
    assert (r["its"], r["reason"]) == (5, ref.ITS)
    r = ref.bcgs_ref(O, np.zeros(b.size))
    assert (r["its"], r["reason"]) == (0, ref.ATOL) and not r["x"].any()
    with pytest.raises(ValueError):
        ref.bcgs_ref(O, b, norm="unpreconditioned")
