"""Time the free-S iteration with the smoothness prior (solve(smooth=...)) against the iteration
without it on one build, at the C3 shape and inputs (bench.py's BASELINE recipe: 512 x 512 x 256,
R = 8, f = 0.1, seed 20263; the same Y, mask and starting point for all), with HIP events on the
replay stream; prints one JSON line.

Solvers: "fused" (smooth = 0, the default two-launch iteration), "unfused" (smooth = 0,
fuse=False: cpass, cfinish, spass), "quad" and "huber" (smooth > 0: cpass, cfinish, spass mode 0,
qsc_smooth_grad, qsc_supdate).  All are built and warmed first; then ROUNDS rounds alternate them,
each round one prepared hipGraph replay of ITERS outer iterations behind LEAD untimed ones, as
tools/bench_logit.py does.  qsc_smooth_grad alone (its gradient kernel and one-block finish) is
timed the same way as a captured graph of CALLS back-to-back calls on the solver's S, and set
against the HBM time of its algorithmic bytes (S read, dS read and written,
the neighbour table read, four gathered neighbour rows per position).

  python tools/bench_smooth.py [--iters 200] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantized_spectrum_cartography_amd import synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402
from quantized_spectrum_cartography_amd.qmc import FreeSSolver  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
LEAD = 8
CALLS = 100
HBM_BYTES_PER_S = 6.3e12  # achievable HBM3E rate on MI355X (8 TB/s peak)


def timed(sol, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    sol.run(LEAD, use_graph=True)  # untimed: runs while the host submits the timed replay
    e0.record()
    sol.run(iters, use_graph=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per outer iteration


def kernel_graph(sol, kind, delta):
    """A captured graph of CALLS qsc_smooth_grad calls on the solver's S and gradient buffer."""
    e = sol.engine
    dS = torch.zeros_like(sol.S)
    e.smooth_grad(sol.S, dS, kind, delta, 1.0, record=False)  # (buffers and table exist)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                e.smooth_grad(sol.S, dS, kind, delta, 1.0, record=False)
    torch.cuda.current_stream().wait_stream(s)
    return g, dS


def timed_graph(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    g.replay()  # untimed lead
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--smooth", type=float, default=1.0)
    ap.add_argument("--delta", type=float, default=0.05)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    configs = {"fused": dict(), "unfused": dict(fuse=False),
               "quad": dict(smooth=args.smooth),
               "huber": dict(smooth=args.smooth, smooth_kind="huber", smooth_delta=args.delta)}
    sols = {}
    for name, kw in configs.items():
        obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
        sol = FreeSSolver(obs, prob["S0"], prob["C0"], **kw)
        assert sol.fuse == (name == "fused")
        sol.run(4, use_graph=True)
        sol.prepare(args.iters)
        sol.prepare(LEAD)
        sols[name] = sol
    graphs = {"quad": kernel_graph(sols["quad"], "quad", None),
              "huber": kernel_graph(sols["huber"], "huber", args.delta)}
    times = {k: [] for k in sols}
    ktimes = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, sol in sols.items():
            times[name].append(timed(sol, args.iters))
        for name, (g, _) in graphs.items():
            ktimes[name].append(timed_graph(g))
    Pp, RP = sols["quad"].S.shape
    row = RP * 4
    nbytes = Pp * (row + 2 * row + 16 + 4 * row)  # S, dS read + write, nbr, 4 gathered rows
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": Pp, "RP": RP,
                     "nnz": int(sols["fused"].obs.nnz)},
           "iters_per_round": args.iters, "rounds": args.rounds, "smooth": args.smooth,
           "delta": args.delta, "us_per_iter": {k: stats(t) for k, t in times.items()},
           "smooth_grad": {"calls_per_graph": CALLS, "algorithmic_bytes": nbytes,
                           "hbm_floor_us": nbytes / HBM_BYTES_PER_S * 1e6}}
    for name, t in ktimes.items():
        st = stats(t)
        st["hbm_roofline_fraction"] = out["smooth_grad"]["hbm_floor_us"] / st["median"]
        out["smooth_grad"][name + "_us_per_call"] = st
    u = out["us_per_iter"]
    out["quad_over_unfused_time"] = u["quad"]["median"] / u["unfused"]["median"]
    out["quad_over_fused_time"] = u["quad"]["median"] / u["fused"]["median"]
    out["huber_over_unfused_time"] = u["huber"]["median"] / u["unfused"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
