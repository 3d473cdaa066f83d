#!/usr/bin/env python3
"""Device time of the annealed chains of the log partition function (k_ais.hip) against the plain Metropolis chains (k_sample.hip) at
the same number of workgroups and proposals, on the model of tests/golden/reference/small.fasta.gz (N = 53, q = 21) resident in HBM:
gdca_log_partition_dev with K = 4096, L = 200, sweep = 53 against gdca_sample_dev with the same K and burn + n_samples stride = 10600
proposals at beta = 1 from the annealed chains' own starts.  Three calls alternate in one process:

    ais       the ladder np.linspace(0, 1, L + 1);
    ais_flat  the ladder (0, 1, 1, .., 1): every proposal at beta = 1 from the same starts on the same streams, so the chains make the
              moves of the plain chains one for one -- the two kernels on identical work;
    sample    gdca_sample_dev, code the annealed chains do not touch.

Reported: the medians of the repeats (HIP events on the stream the context works on; every call includes its start tables), the spread
of each, the acceptance of each, and what an annealed call pays around its chain launches -- the ladder's upload, k_ais_start, the
start energies, the start tables, k_ais_reduce -- as the time of a call of ONE proposal (L = 1, sweep = 1), beside the same for the
plain chains.  Every GPU step runs under a time limit of its own.

    python tools/ais_bench.py --out profiles/ais_bench.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

from mutation_bench import step_limit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--sweep", type=int, default=53)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ais_bench.json"))
    args = ap.parse_args()

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops

    K, L, sweep, q = args.K, args.L, args.sweep, 21
    T = L * sweep
    Z = gd.read_fasta_alignment(os.path.join(ROOT, "tests", "golden", "reference", "small.fasta.gz"), 0.9)  # (N, M), Fortran order
    N, M = Z.shape
    n = N * (q - 1)
    stream = torch.cuda.current_stream()
    with step_limit(60, "context"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    with step_limit(120, "operator chain"):
        dZ = torch.from_numpy(np.ascontiguousarray(Z.T)).cuda()
        dPi = torch.empty(n, dtype=torch.float64, device="cuda")
        dmJ = torch.empty(n * n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dW, Meff, _, _ = devops.compute_weights_dev(ctx, dZ.data_ptr(), N, M, ":auto")
        devops.compute_weighted_frequencies_dev(ctx, dZ.data_ptr(), N, M, q, dW, Meff, dPi.data_ptr(), dmJ.data_ptr())
        devops.add_pseudocount_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), N, q, args.pseudocount)
        devops.compute_C_dev(ctx, dPi.data_ptr(), dmJ.data_ptr(), n, dC=dmJ.data_ptr())
        devops.inv_cholesky_dev(ctx, dmJ.data_ptr(), n)
        ctx.synchronize()
    with step_limit(60, "buffers"):
        dout = torch.empty(4, dtype=torch.float64, device="cuda")
        dlogw = torch.empty(K, dtype=torch.float64, device="cuda")
        dX0 = torch.empty((K, N), dtype=torch.int8, device="cuda")
        dXs = torch.empty((K, N), dtype=torch.int8, device="cuda")
        dacc = torch.empty(K, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    ladder = np.linspace(0.0, 1.0, L + 1)
    flat = np.concatenate(([0.0], np.ones(L)))

    def ais(betas, sw=sweep):  # every site free, the gap a symbol; the starts and the counts come back
        ctx.log_partition_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, None, None, gd._lib.SAMPLE_GAPS, betas, sw, K, 1, 0, dout.data_ptr(),
                              dlogw.data_ptr(), None, dX0.data_ptr(), None, dacc.data_ptr())

    def sample(steps=T):  # from the annealed chains' starts (seed and streams are the same for every call: dX0 does not change)
        ctx.sample_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX0.data_ptr(), K, None, gd._lib.SAMPLE_GAPS, 1.0, 1, 0, steps - 1, 1, 1, dXs.data_ptr(),
                       dacc.data_ptr())

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def acceptance(steps=T):
        return float(dacc.cpu().numpy().astype(np.int64).sum()) / (K * steps)

    calls = (("ais", lambda: ais(ladder)), ("ais_flat", lambda: ais(flat)), ("sample", sample),
             ("ais_one_proposal", lambda: ais(np.array([0.0, 1.0]), 1)), ("sample_one_proposal", lambda: sample(1)))
    ms = {name: [] for name, _ in calls}
    acc = {}
    with step_limit(900, "the alternating calls"):
        for r in range(args.warmup + args.repeats):
            for name, fn in calls:
                t = once(fn)
                if r >= args.warmup:
                    ms[name].append(t)
                if r == 0:
                    acc[name] = acceptance(1 if "one_proposal" in name else T)
        ais(flat)
        ctx.synchronize()
        acc_flat = dacc.cpu().numpy().copy()
        sample()
        ctx.synchronize()
        same_moves = bool(np.array_equal(acc_flat, dacc.cpu().numpy()))
        out4 = dout.cpu().numpy().tolist()
    ctx.close()

    med = {name: statistics.median(v) for name, v in ms.items()}
    res = dict(model="small.fasta.gz", N=N, M=M, q=q, K=K, L=L, sweep=sweep, n_steps=T, flags="GAPS, every site free", repeats=args.repeats,
               warmup=args.warmup, ms=med, ms_all=ms, spread={name: (max(v) - min(v)) / med[name] for name, v in ms.items()}, acceptance=acc,
               flat_ladder_makes_the_plain_chains_moves=same_moves, ratio_ais_to_sample=med["ais"] / med["sample"],
               ratio_flat_to_sample=med["ais_flat"] / med["sample"],
               chains_only_ratio_flat_to_sample=(med["ais_flat"] - med["ais_one_proposal"]) / (med["sample"] - med["sample_one_proposal"]),
               out4_of_the_last_flat_call=out4)
    print("ais %.2f ms (acceptance %.3f), flat ladder %.2f ms (%.3f), sample %.2f ms (%.3f); one proposal: ais %.3f ms, sample %.3f ms; "
          "flat / sample %.4f, spreads %.4f / %.4f, the same moves: %s"
          % (med["ais"], acc["ais"], med["ais_flat"], acc["ais_flat"], med["sample"], acc["sample"], med["ais_one_proposal"],
             med["sample_one_proposal"], res["ratio_flat_to_sample"], res["spread"]["ais_flat"], res["spread"]["sample"], same_moves), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
