#!/usr/bin/env python3
"""BiCGStab + Jacobi against GMRES(30) + Jacobi on the convection-diffusion
operator (C4: 256^3, and 128^3 where the GMRES basis is small), hash
right-hand side, rtol 1e-5, one GPU.  Recorded, not gated.

    python tools/bcgs_vs_gmres.py [--sizes 128,256] [--out out/bcgs_c4.json] [--timeout 240]

Every solve runs in a process of its own under a time limit; after one that
fails or runs out of time nothing more is started.  One JSON line per solve:
its, reason, solve_ms (device time of a plain solve), the per-pass times of a
second, profiled solve, the true relative residual ||b - A x|| / ||b||, and
for the timed BiCGStab passes the bytes model's rate as a fraction of 8 TB/s.
A last line per size times cg_pb_kernel (CG on the 7-point Poisson operator of
the same size) for comparison, and a summary line gives the time-to-solution
ratio."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-petsc4py-example_amd"))
PEAK = 8.0e12   # bytes / s


def one(ksp: str, n: int) -> dict:
    import torch  # noqa: F401
    from mxsolve.core import DeviceComm, DMat, rhs_hash, vaypx, vnorm
    comm = DeviceComm.self_comm(0)
    cgpb = ksp == "cgpb"
    A = DMat.stencil(comm, "poisson3d" if cgpb else "convdiff3d", n)
    m = A.info()["m"]
    b = comm.empty(m)
    rhs_hash(comm, 0, b)
    x = comm.zeros(m)
    if cgpb:       # the comparison figure: CG's batched direction update
        A.solve(b, x, ksp="cg", pc="jacobi", rtol=0.0, max_it=16)
        r = A.solve(b, x, ksp="cg", pc="jacobi", rtol=0.0, max_it=64, profile=4)
        B = max(r["cg_xbatch"], 1)
        # doubles per row of a launch: r, p_{i-1} -> p_i (3); an x-step batch reads
        # r, B directions and x and writes x and p_i (B + 4).  Only the batches
        # go through cg_pb_kernel when the other iterations' direction update
        # rides in the p.Ap pass (pb_count == iterations / B)
        only_batches = B > 1 and r["pb_count"] * B == r["launched_its"]
        doubles = 3.0 if B == 1 else (B + 4.0 if only_batches else ((B - 1) * 3 + B + 4) / B)
        ms = r["pb_ms"] / max(r["pb_count"], 1)
        out = {"pass": "cg_pb_kernel", "n": n, "cg_mode": r["cg_mode"], "cg_xbatch": B, "launches": r["pb_count"],
               "ms_per_launch": ms, "doubles_per_row": doubles,
               "frac_of_8TBs": doubles * 8 * m / (ms * 1e-3) / PEAK if ms > 0 else None}
        A.destroy()
        return out
    kw = dict(ksp=ksp, pc="jacobi", rtol=1e-5, restart=30)
    A.solve(b, x, max_it=8, **kw)                       # code objects, work space, Jacobi setup
    r = A.solve(b, x, **kw)
    y = comm.empty(m)
    A.mult(x, y)
    vaypx(comm, -1.0, b, y)                             # y = b - A x
    true_rel = vnorm(comm, y) / vnorm(comm, b)
    x2 = comm.zeros(m)
    q = A.solve(b, x2, profile=7, **kw)
    out = {"ksp": ksp, "n": n, "rows": m, "its": r["its"], "reason": r["reason"], "solve_ms": r["solve_ms"],
           "its_per_s": r["its"] / (r["solve_ms"] * 1e-3) if r["solve_ms"] > 0 else None,
           "rnorm": r["rnorm"], "true_rel_residual": true_rel, "launched_its": r["launched_its"],
           "profiled": {"its": q["its"], "solve_ms": q["solve_ms"],
                        "spmv_ms": q["spmv_ms"], "spmv_count": q["spmv_count"]}}
    p = out["profiled"]
    if ksp == "bcgs":
        p.update(bcgs_xr_ms=q["upd_ms"], bcgs_xr_count=q["upd_count"], bcgs_p_ms=q["pb_ms"], bcgs_p_count=q["pb_count"])
        # (launches past the stop are no-ops of a few microseconds: the passes' time is the its iterations')
        for name, doubles, ms in (("bcgs_xr", 7, q["upd_ms"]), ("bcgs_p", 4, q["pb_ms"])):
            if q["its"] and ms > 0:
                p[name + "_ms_per_it"] = ms / q["its"]
                p[name + "_frac_of_8TBs"] = doubles * 8 * m / (ms / q["its"] * 1e-3) / PEAK
    else:
        p.update(mdot_ms=q["mdot_ms"], mdot_count=q["mdot_count"], maxpy_ms=q["maxpy_ms"], maxpy_count=q["maxpy_count"])
    if p["spmv_count"]:
        p["spmv_ms_per_launch"] = p["spmv_ms"] / p["spmv_count"]
    out["ms_per_it"] = r["solve_ms"] / max(r["its"], 1)
    A.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("KSP", "N"), help="(internal) one solve in this process")
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--out", default=os.path.join(os.environ.get("MX_OUT", "out"), "bcgs_c4.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per solve")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], int(a.one[1]))), flush=True)
        return 0
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n in (int(s) for s in a.sizes.split(",")):
        got = {}
        for ksp in ("gmres", "bcgs", "cgpb"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", ksp, str(n)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                print(json.dumps({"failed": ksp, "n": n, "returncode": res.returncode}), flush=True)
                return 1                      # start nothing more on the GPU
            line = res.stdout.strip().splitlines()[-1]
            got[ksp] = json.loads(line)
            lines.append(line)
            print(line, flush=True)
        ratio = {"summary": "time to solution", "n": n, "gmres_ms": got["gmres"]["solve_ms"],
                 "bcgs_ms": got["bcgs"]["solve_ms"], "bcgs_over_gmres": got["bcgs"]["solve_ms"] / got["gmres"]["solve_ms"]}
        lines.append(json.dumps(ratio))
        print(lines[-1], flush=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
