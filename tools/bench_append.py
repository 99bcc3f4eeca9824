"""Time Observations.append at the C3 shape (bench.py's BASELINE recipe: 512 x 512 x 256, R = 8,
f = 0.1, seed 20263: 6.71 M readings, packed as a list) against the route it replaces, for two
batches: 1 % of n readings at random cells, and one planned batch of 64 sites x K readings.

End to end (wall clock, synchronised, in one session, alternating): obs.append(batch), the merge,
against readings() + cat + from_readings(perm=obs.perm, tile=...), the re-sort.  Median, min - max
and spread (max - min over the rounds) of each.
The merge call alone: qsc_obs_readings_merge (synchronous: the batch's sort, the two placements
and merges, the layout stages and the read-back of the totals) on preallocated buffers, against
the HBM time of the merge's algorithmic bytes: 8 n in and 8 (n + m) out for the two sorted arrays
plus the five tables of `packed` in and out.
The merge kernels alone (--trace): the call is synchronous, so it cannot be replayed from a graph;
before this process touches the GPU the tool starts
    rocprofv3 --kernel-trace --stats --output-format csv -d TMP -o append -- \
        python tools/bench_append.py --rounds 2 --out TMP/traced.json
as a child, reads TMP/**/append_kernel_stats.csv and records calls, average, min and max of
merge_kernel, ins_kernel and ccount_init_kernel under "kernels_ns", merge_kernel against its own
algorithmic bytes (4 n in, 4 (n + m) out per sorted array).
Prints one JSON line and writes it to profiles/append/bench_append_c3.json.

  python tools/bench_append.py [--rounds 7] [--trace] [--out profiles/append/bench_append_c3.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_spectrum_cartography_amd import _lib, synthetic  # noqa: E402
from quantized_spectrum_cartography_amd.obs import Observations  # noqa: E402

SEED = 20260 + 3  # bench.py's C3 seed
FRAC = 0.1
SITES = 64
HBM_BYTES_PER_S = 6.3e12  # achievable HBM3E rate on MI355X (8 TB/s peak)


KERNELS = ("merge_kernel", "ins_kernel<true>", "ins_kernel<false>", "ccount_init_kernel")
TRACE_ROUNDS = 2


def kernel_trace():
    """The statistics of the merge's kernels from a kernel trace of a child run of this script
    (TRACE_ROUNDS rounds, both batches).  Called before this process uses the GPU."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("--trace needs rocprofv3 on the PATH")
    tmp = tempfile.mkdtemp(prefix="bench_append_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o",
               "append", "--", sys.executable, os.path.abspath(__file__), "--rounds",
               str(TRACE_ROUNDS), "--out", os.path.join(tmp, "traced.json")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=400)
        files = glob.glob(os.path.join(tmp, "**", "append_kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit("rocprofv3 left %d kernel statistics files" % len(files))
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for name in KERNELS:
                    if "::" + name + "(" in row["Name"]:
                        out[name] = {"calls": int(row["Calls"]), "average": float(row["AverageNs"]),
                                     "min": int(row["MinNs"]), "max": int(row["MaxNs"])}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3  # ms


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t), "spread": max(t) - min(t)}


def merge_call(obs, k, i, j, c):
    """(a closure that runs qsc_obs_readings_merge alone on preallocated buffers, its
    algorithmic bytes)."""
    K, P, PT, n, m = obs.K, obs.P, int(obs.desc.PT), obs.nnz, k.numel()
    kd, pd, cd = Observations._device_readings(k, i, j, c, obs.I, obs.J)
    bcnt = torch.empty(P, dtype=torch.int32, device=obs.device)
    bad = torch.zeros(1, dtype=torch.int32, device=obs.device)
    _lib.call("qsc_obs_readings_count", _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), 1, m, K, P,
              int(obs.desc.nbins), _lib.ptr(bcnt), _lib.ptr(bad), _lib.stream())
    assert int(bad.item()) == 0
    cnt = obs.counts + bcnt
    new = obs._child()
    new._alloc_tables(PT)
    L = _lib.lib()
    nb = L.qsc_obs_readings_merge_packed_bytes(n, m, K, P, PT)
    wb = L.qsc_obs_readings_merge_workspace_bytes(n, m, K, P, PT)
    out = torch.empty(nb, dtype=torch.uint8, device=obs.device)
    ws = torch.empty(wb, dtype=torch.uint8, device=obs.device)
    desc = _lib.QscObsDesc()

    def run():
        rep = ctypes.c_int32(int(obs.max_repeat))
        _lib.call("qsc_obs_readings_merge", _lib.ptr(obs._packed), obs._packed.numel(), n,
                  obs.desc, _lib.ptr(obs.perm), _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), 1, m,
                  _lib.ptr(cnt), _lib.ptr(new.s_width), _lib.ptr(new.s_off), _lib.ptr(new.c_width),
                  _lib.ptr(new.c_off), _lib.ptr(new.c_kmap), _lib.ptr(out), nb, _lib.ptr(ws), wb,
                  desc, ctypes.byref(rep), _lib.stream())
    tables = obs._packed.numel() - 8 * n
    return run, 8 * n + 8 * (n + m) + 2 * tables, wb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append",
                                                  "bench_append_c3.json"))
    ap.add_argument("--trace", action="store_true",
                    help="also record the merge kernels' own times from a rocprofv3 child run")
    args = ap.parse_args()
    kernels = kernel_trace() if args.trace else None
    if not torch.cuda.is_available():
        raise SystemExit("bench_append.py needs an MI355X: nothing is timed without one")
    I, J, K, R = 512, 512, 256, 8
    prob = synthetic.onebit_problem(I, J, K, R, f=FRAC, seed=SEED)
    b, sigma = prob["b"], prob["sigma"]
    dense = Observations(prob["Y"], prob["Wx"], b, sigma, R_hint=R)
    obs = Observations.from_readings(*(t.clone() for t in dense.readings()), (K, I, J), b, sigma,
                                     R_hint=R, perm=dense.perm, tile=dense.desc.PT)
    del dense
    n, dev = obs.nnz, obs.device
    g = torch.Generator(device="cpu").manual_seed(1)
    m1 = n // 100
    sites = torch.randperm(I * J, generator=g)[:SITES]
    batches = {
        "one_percent": (torch.randint(0, K, (m1,), generator=g), torch.randint(0, I, (m1,), generator=g),
                        torch.randint(0, J, (m1,), generator=g),
                        torch.randint(0, 2, (m1,), generator=g).to(torch.uint8)),
        "planned_64_sites": (torch.arange(K).repeat(SITES), (sites // J).repeat_interleave(K),
                             (sites % J).repeat_interleave(K),
                             (torch.arange(SITES * K) % 2).to(torch.uint8))}
    batches = {name: tuple(t.to(dev) for t in v) for name, v in batches.items()}

    def resort_of(batch):
        def run():
            parts = [torch.cat((a, x.to(a.dtype))) for a, x in zip(obs.readings(), batch)]
            return Observations.from_readings(*parts, (K, I, J), b, sigma, R_hint=R, perm=obs.perm,
                                              tile=obs.desc.PT)
        return run

    res = {"shape": {"I": I, "J": J, "K": K, "readings": n, "tile": int(obs.desc.PT)},
           "rounds": args.rounds, "batches": {}}
    for name, batch in batches.items():
        m = batch[0].numel()
        call, nbytes, wb = merge_call(obs, *batch)
        fns = {"append": lambda batch=batch: obs.append(*batch), "resort_route": resort_of(batch),
               "merge_call": call}
        a, r = fns["append"](), fns["resort_route"]()  # untimed lead; the same packing
        assert a.nnz == r.nnz == n + m and torch.equal(a.s_entries, r.s_entries)
        assert torch.equal(a.c_entries, r.c_entries) and torch.equal(a.c_kmap, r.c_kmap)
        del a, r
        fns["merge_call"]()
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t[k].append(wall(fn))
        ms = {k: stats(v) for k, v in t.items()}
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        ms["merge_call"].update(algorithmic_bytes=nbytes, hbm_floor_ms=floor_ms,
                                hbm_roofline_fraction=floor_ms / ms["merge_call"]["median"],
                                workspace_bytes=wb)
        sep = (ms["append"]["max"] < ms["resort_route"]["min"] or
               ms["resort_route"]["max"] < ms["append"]["min"])
        res["batches"][name] = {
            "m": m, "ms": ms,
            "append_over_resort": ms["append"]["median"] / ms["resort_route"]["median"],
            "winner": ("append" if ms["append"]["median"] < ms["resort_route"]["median"]
                       else "resort_route"),
            "outside_both_spreads": bool(sep)}
    if kernels is not None:
        ms_ = [b["m"] for b in res["batches"].values()]
        lo, hi = 4 * n + 4 * (n + min(ms_)), 4 * n + 4 * (n + max(ms_))
        if "merge_kernel" in kernels:
            kernels["merge_kernel"].update(
                algorithmic_bytes_per_call=[lo, hi],
                hbm_floor_ns=[lo / HBM_BYTES_PER_S * 1e9, hi / HBM_BYTES_PER_S * 1e9],
                hbm_roofline_fraction=hi / HBM_BYTES_PER_S * 1e9 / kernels["merge_kernel"]["average"])
        res["kernels_ns"] = {"source": "rocprofv3 --kernel-trace --stats, a child run of %d rounds "
                             "over both batches" % TRACE_ROUNDS, **kernels}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
