"""Time the per-bin projected Newton fit of C (qsc_cfit_*) at the C3 shape and inputs (bench.py's
BASELINE recipe: 512 x 512 x 256, R = 8, f = 0.1, seed 20263) with the S and C of a standard solver
run, with HIP events around replays of captured graphs of CALLS back-to-back fits (the protocol of
tools/bench_sfit.py: one untimed lead replay, ROUNDS alternating rounds).

  (a) the time of one walk + step, by differencing max_steps = 1 and 3 with a tolerance no step
      meets (so that no bin stops early), next to qsc_cpass in the same session (the same lists,
      first order only) and to the HBM time of the walk's algorithmic bytes;
  (b) the full fit_C from C = 0 with the defaults (never syncing): the histogram of steps and the
      total time.
Prints one JSON line and writes it to profiles/cfit/bench_cfit_c3.json.

  python tools/bench_cfit.py [--rounds 7] [--iters 200] [--out profiles/cfit/bench_cfit_c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, qmc, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
CALLS = 4
HBM_GBPS = 8000.0  # MI355X peak HBM3E bandwidth (the figure DESIGN.md's rooflines use)


def capture(fn):
    """A captured graph of CALLS back-to-back calls of fn (called once eagerly first)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


def timed_graph(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    g.replay()  # untimed lead
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200, help="solver iterations that produce S, C")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfit", "bench_cfit_c3.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cfit.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=0.1, seed=SEED)
    obs = Observations(prob["Y"], prob["Wx"], prob["b"], prob["sigma"], R_hint=R)
    sol = qmc.FreeSSolver(obs, prob["S0"], prob["C0"])
    sol.run(args.iters)
    torch.cuda.synchronize()
    C = sol.C.clone()
    S_pos = sol.S.clone()
    ridge = qmc.default_confidence_ridge(C, 100.0)
    desc, _, c_entries = obs.layout(R)
    RP = obs.rank_pad(R)
    C0 = torch.zeros_like(C)
    C_out = torch.empty_like(C)
    p = _lib.ptr
    nws = int(_lib.lib().qsc_cfit_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    pws_n = int(_lib.lib().qsc_pass_workspace_bytes(desc, R))
    pws = torch.zeros(pws_n, dtype=torch.uint8, device="cuda")

    def cpass():
        _lib.call("qsc_cpass", desc, p(c_entries), p(obs.c_width), p(obs.c_off), p(obs.c_kmap),
                  obs.model, R, p(S_pos), p(C), p(pws), pws_n, _lib.stream())

    def cfit(max_steps, tol, init):
        qmc._fit_c_pos(obs, S_pos, init, R, "observed", ridge, max_steps, tol, 1e-3, True,
                       sync_every=0, C_out=C_out, ws=ws)

    graphs = {"cpass": capture(cpass),
              "cfit_steps1": capture(lambda: cfit(1, 1e-30, C)),
              "cfit_steps3": capture(lambda: cfit(3, 1e-30, C)),
              "cfit_full": capture(lambda: cfit(30, 1e-5, C0))}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(timed_graph(g))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = qmc.fit_C(obs, sol.S_pixels(), ridge=ridge)
    hist = torch.bincount(res.steps.long()).tolist()
    per_iter = (med["cfit_steps3"] - med["cfit_steps1"]) / 2.0
    NA = (RP + RP * (RP + 1) // 2 + 3) // 4 * 4  # a partial row: g, the triangle of J, padded
    G = int(_lib.lib().qsc_cfit_groups(desc, R))
    # algorithmic bytes of one walk + step: the entries and S once, the partials written and read
    walk_bytes = (int(desc.c_entries) * obs.entry_bytes + obs.Pp * RP * 4
                  + 2 * G * K * (NA * 4 + 8))
    out = {"shape": {"I": I, "J": J, "K": K, "R": R, "Pp": obs.Pp, "RP": RP, "PT": int(desc.PT),
                     "ntiles": int(desc.ntiles), "nks": int(desc.nks), "nnz": int(obs.nnz),
                     "c_entries": int(desc.c_entries), "rowfmt": int(desc.rowfmt),
                     "workspace_bytes": nws, "groups": G},
           "solver_iters_for_S_C": args.iters, "ridge": ridge, "calls_per_graph": CALLS,
           "rounds": args.rounds,
           "us_per_call": {k: {"median": med[k], "min": min(v), "max": max(v)}
                           for k, v in times.items()},
           "us_per_walk_and_step": per_iter,
           "walk_and_step_over_cpass": per_iter / med["cpass"],
           "walk_algorithmic_bytes": walk_bytes,
           "hbm_us_of_those_bytes": walk_bytes / (HBM_GBPS * 1e3),
           "full_fit": {"us": med["cfit_full"], "steps_histogram": hist, "nll": res.nll,
                        "unconverged": res.unconverged, "unidentified": res.unidentified}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
