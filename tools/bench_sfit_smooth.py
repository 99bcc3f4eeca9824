"""Time the red-black Newton fit qsc_sfit_smooth at the C3 shape and inputs (bench.py's BASELINE
recipe: 512 x 512 x 256, R = 8, f = 0.1, seed 20263) with the S and C of a solver run with the
smoothness prior, with HIP events around replays of captured graphs of CALLS back-to-back calls
(the protocol of tools/bench_sfit.py: one untimed lead replay, ROUNDS alternating rounds).

  (a) the time of one sweep at inner_steps = 1 (two launches of two walks each), by differencing
      1 and 3 sweeps at a tolerance nothing meets, against one walk-and-solve iteration of
      qsc_sfit in the same session (max_steps 1 and 3 differenced, as tools/bench_sfit.py);
      the structure predicts a ratio of about 4 (four walks, half of the lanes idle in each);
  (b) the full fit_S_smooth with the defaults: its time, sweep count and `moved`.
Prints one JSON line and writes it to profiles/sfit_smooth/bench_sfit_smooth_c3.json.

  python tools/bench_sfit_smooth.py [--rounds 7] [--iters 200] [--smooth 0.1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_sfit import CALLS, SEED, capture, timed_graph  # noqa: E402
from quantized_spectrum_cartography_amd import qmc, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200, help="solver iterations that produce S, C")
    ap.add_argument("--smooth", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfit_smooth",
                                                  "bench_sfit_smooth_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sfit_smooth.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    sol = qmc.FreeSSolver(obs, prob["S0"], prob["C0"], smooth=args.smooth)
    sol.run(args.iters)
    torch.cuda.synchronize()
    C = sol.C.clone()
    S_sol = sol.S.clone()  # position order
    S_pix = sol.S_pixels()
    ridge = qmc.default_confidence_ridge(S_pix, 100.0)
    S_work = torch.empty_like(S_sol)
    S_out = torch.empty_like(S_sol)
    obs.neighbors()

    def sweeps(n, inner, tol):
        S_work.copy_(S_sol)
        qmc._fit_s_smooth_pos(obs, S_work, C, R, "observed", ridge, n, inner, tol, 1e-3, False,
                              "quad", None, args.smooth, sync_every=0)

    def sfit(max_steps, tol):
        qmc._fit_s_pos(obs, S_sol, C, R, "observed", ridge, max_steps, tol, 1e-3, False,
                       S_out=S_out)

    graphs = {"sweeps1": capture(lambda: sweeps(1, 1, 1e-30)),
              "sweeps3": capture(lambda: sweeps(3, 1, 1e-30)),
              "sfit_steps1": capture(lambda: sfit(1, 1e-30)),
              "sfit_steps3": capture(lambda: sfit(3, 1e-30))}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(timed_graph(g))
    med = {k: statistics.median(v) for k, v in times.items()}
    per_sweep = (med["sweeps3"] - med["sweeps1"]) / 2.0
    per_iter = (med["sfit_steps3"] - med["sfit_steps1"]) / 2.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = qmc.fit_S_smooth(obs, C, args.smooth, S_init=S_pix, ridge=ridge)
    torch.cuda.synchronize()
    full_s = time.perf_counter() - t0
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": obs.Pp, "nnz": int(obs.nnz)},
           "solver_iters": args.iters, "smooth": args.smooth, "ridge": ridge,
           "calls_per_graph": CALLS, "rounds": args.rounds,
           "us_per_call": {k: {"median": med[k], "min": min(v), "max": max(v)}
                           for k, v in times.items()},
           "us_per_sweep_inner1": per_sweep, "us_per_sfit_iteration": per_iter,
           "sweep_over_sfit_iteration": per_sweep / per_iter,
           "full_fit": {"wall_ms": full_s * 1e3, "sweeps": res.sweeps, "moved": res.moved,
                        "unidentified": res.unidentified, "objective": res.objective,
                        "nll": res.nll, "penalty": res.penalty}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
