#!/usr/bin/env python3
"""Device time of partner matching per species (k_pair_gather_blocked, k_assign_blocks) at the two shapes of DESIGN 3.7, species of
1..32 sequences a side from a fixed SplitMix64 stream:
  (a) the blocked energy stage on a resident mJ (gdca_pair_energies_blocked_dev),
  (b) the full K_A x K_B matrix on the same sequences (gdca_pair_energies_dev), measured again in this process,
  (c) a loop of one gdca_pair_energies_dev call per species,
  (d) the assignment alone (gdca_assign_blocks_dev) -- and scipy.optimize.linear_sum_assignment on the downloaded blocks (host time),
  (e) ms_score / ms_total of the fused run (gdca_run_partner_match_dev),
  (f) the floor: the fold unchanged, T written and read once, the packed symbols, the blocks written once, at k_fn20's HBM rate; the
      LDS row reads of the fold and of the blocked gather at 128 bytes a clock a compute unit, no bank conflict assumed.
Two conditions are work arguments and are checked: (a) <= (b) -- the same fold, strictly less gather -- and (a) < (c).  One process;
contexts are made before anything is timed; HIP events on the stream the context works on, 10 timed repeats after 2, medians; every
GPU step under a time limit of its own (a step that overruns ends the process with status 124, nothing is started after it).

    python tools/partner_bench.py --config B --out profiles/partner_bench.json   (N = 128, split = 64, M = 10 000, K_A = K_B = 4096)
    python tools/partner_bench.py --config C --out profiles/partner_bench.json   (N = 500, split = 250, M = 50 000, K_A = K_B = 8192)
Results of several configs are merged into one JSON file by config name."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

CONFIGS = {"B": dict(N=128, split=64, M=10000, K=4096, theta=0.2, seed=0xB128),
           "C": dict(N=500, split=250, M=50000, K=8192, theta=-1.0, seed=0xC500)}
PEAK_HBM = 8.0e12                  # bytes / s
FN_HBM_FRACTION = (0.58, 0.64)     # what k_fn20 reaches streaming the same matrix
CUS, GHZ, LDS_BYTES_PER_CLK = 256, 2.4, 128


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("partner_bench: step '%s' exceeded %d s\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(seconds, over)
    t.daemon = True
    t.start()
    try:
        yield
    finally:
        t.cancel()


def timed(fn, warmup, repeats):
    """HIP events on the current torch stream (the context was made on it) -> list of ms"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def species_sizes(K, seed=0x5EC1E5):
    """sizes in 1..32 from a SplitMix64 stream until they hold K sequences (the last one cut)"""
    mask, state, sizes, total = (1 << 64) - 1, seed, [], 0
    while total < K:
        state = (state + 0x9E3779B97F4A7C15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        k = min(1 + int(z % 32), K - total)
        sizes.append(k)
        total += k
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partner_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, split, M, K, q, theta, pc = c["N"], c["split"], c["M"], c["K"], 21, c["theta"], args.pseudocount
    s = q - 1
    n, nA, nB, NA, NB = N * s, split * s, (N - split) * s, split, N - split
    ENERGY = gd._lib.PAIR_ENERGY
    sizes = species_sizes(K)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    S, pairings = len(sizes), int(sum(k * k for k in sizes))
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dXA = dZ[:K, :split].contiguous()   # column-major split x K
        dXB = dZ[:K, split:].contiguous()
        dE = torch.empty(K * K, dtype=torch.float64, device="cuda")
        dEb = torch.empty(pairings, dtype=torch.float64, device="cuda")
        dmatch = torch.empty(K, dtype=torch.int32, device="cuda")
        dgap = torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, split=split, M=M, KA=K, KB=K, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats,
               warmup=args.warmup, species=S, pairings=pairings, largest_species=max(sizes))

    # ---- (e) the fused run: ms_score is the blocked pair stage plus the assignment
    with step_limit(300, "gdca_run_partner_match"):
        sts = []
        for i in range(args.warmup + args.repeats):
            st = ctx.run_partner_match_dev(dZ.data_ptr(), N, M, q, pc, theta, split, dXA.data_ptr(), K, dXB.data_ptr(), K, off, off, ENERGY,
                                           dEb.data_ptr(), dmatch.data_ptr(), dgap.data_ptr())
            if i >= args.warmup:
                sts.append(st)
        res["fused_ms_total"] = statistics.median(x["ms_total"] for x in sts)
        res["fused_ms_score"] = statistics.median(x["ms_score"] for x in sts)
        res["fused_ms_score_all"] = [x["ms_score"] for x in sts]
        match_fused = dmatch.cpu().numpy()

    # ---- the operators on a resident mJ (built by the library's own device operators)
    with step_limit(180, "operator chain"):
        dPi = torch.empty(n, dtype=torch.float64, device="cuda")
        dmJ = torch.empty(n * n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dW, Meff, _, _ = devops.compute_weights_dev(ctx, dZ.data_ptr(), N, M, theta if theta >= 0 else ":auto")
        devops.compute_weighted_frequencies_dev(ctx, dZ.data_ptr(), N, M, q, dW, Meff, dPi.data_ptr(), dmJ.data_ptr())
        devops.add_pseudocount_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), N, q, pc)
        devops.compute_C_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), n, dC=dmJ.data_ptr())
        devops.inv_cholesky_dev(ctx, dmJ.data_ptr(), n)
        ctx.synchronize()

    def keep(key, ms):
        res[key] = statistics.median(ms)
        res[key + "_all"] = ms

    with step_limit(180, "(a) blocked, (b) full"):
        keep("blocked_ms", timed(lambda: ctx.pair_energies_blocked_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, split, dXA.data_ptr(), K,
                                                                       dXB.data_ptr(), K, off, off, ENERGY, dEb.data_ptr()),
                                 args.warmup, args.repeats))
        keep("full_ms", timed(lambda: ctx.pair_energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, split, dXA.data_ptr(), K, dXB.data_ptr(), K,
                                                            ENERGY, dE.data_ptr()), args.warmup, args.repeats))
        # the blocks against the full matrix of this process: bit for bit
        Eb = dEb.cpu().numpy()
        full = dE.view(K, K).t()   # dE is column-major: [a, b]
        want = np.concatenate([full[off[k]:off[k + 1], off[k]:off[k + 1]].cpu().numpy().ravel(order="F") for k in range(S)])
        res["blocked_equals_full"] = bool(np.array_equal(Eb, want))

    with step_limit(300, "(c) one call per species"):
        pa, pb, pe = dXA.data_ptr(), dXB.data_ptr(), dE.data_ptr()

        def per_species():
            for k in range(S):
                ctx.pair_energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, split, pa + int(off[k]) * split, sizes[k],
                                      pb + int(off[k]) * (N - split), sizes[k], ENERGY, pe)

        keep("per_species_calls_ms", timed(per_species, args.warmup, args.repeats))

    with step_limit(120, "(d) assignment"):
        keep("assign_ms", timed(lambda: ctx.assign_blocks_dev(dEb.data_ptr(), off, off, dmatch.data_ptr(), dgap.data_ptr()), args.warmup,
                                args.repeats))
        match_dev = dmatch.cpu().numpy()
        res["fused_match_equals_operator"] = bool(np.array_equal(match_dev, match_fused))
    ctx.close()

    from scipy.optimize import linear_sum_assignment

    blocks, at = [], 0
    for k in sizes:
        blocks.append(Eb[at:at + k * k].reshape((k, k), order="F"))
        at += k * k
    t0 = time.perf_counter()
    cols = [linear_sum_assignment(b)[1] for b in blocks]
    res["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
    res["match_equals_scipy"] = bool(np.array_equal(match_dev, np.concatenate([cc + o for cc, o in zip(cols, off[:-1])])))
    res["assign_speedup_vs_scipy"] = res["scipy_host_ms"] / res["assign_ms"]

    # ---- (f) the floor.  HBM: the block of mJ, T written by the fold and read by the gather once each, the packed symbols, the
    # marginals' padded sequences, the blocks.  LDS: the fold reads K_A N_A n_B doubles, the blocked gather one double a pairing and
    # site of B.
    res["compulsory_bytes"] = 8.0 * nA * nB + 2 * 8.0 * K * nB + float(N) * 2 * K * 2 + 8.0 * pairings
    res["hbm_ms_at_fn_rate"] = [res["compulsory_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    res["lds_bytes_fold"] = 8.0 * float(K) * NA * nB
    res["lds_bytes_gather"] = 8.0 * float(pairings) * NB
    res["lds_ms_conflict_free"] = (res["lds_bytes_fold"] + res["lds_bytes_gather"]) / (CUS * GHZ * 1e9 * LDS_BYTES_PER_CLK) * 1e3
    res["floor_ms"] = max(min(res["hbm_ms_at_fn_rate"]), res["lds_ms_conflict_free"])
    res["floor_fraction_blocked"] = res["floor_ms"] / res["blocked_ms"]
    res["work_ratio_full_over_blocked"] = float(K) * K / pairings
    res["condition_blocked_le_full"] = bool(res["blocked_ms"] <= res["full_ms"])
    res["condition_blocked_lt_per_species"] = bool(res["blocked_ms"] < res["per_species_calls_ms"])

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}, sort_keys=True))
    ok = res["condition_blocked_le_full"] and res["condition_blocked_lt_per_species"] and res["blocked_equals_full"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
