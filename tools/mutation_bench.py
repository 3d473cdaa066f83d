#!/usr/bin/env python3
"""Device time of the mutation scan (k_mutation.hip) at two shapes and K = 1, 256, 8192 backgrounds: alone on a resident mJ
(gdca_mutation_scan_dev, delta and potential), as ms_score of the fused run (gdca_run_mutation_scan_dev), against its HBM and LDS
floors, against the only route the library had before (gdca_energies_dev on the N q explicit mutants of ONE sequence, SCALED by K:
building and uploading the mutants is not included), and against the obvious torch f64 formulation on the same GPU (one-hot X times
the symmetrised mJ as a dense matmul plus the elementwise epilogue, symmetrising and encoding included).  One process; the context
is made before anything is timed; HIP events on the stream the context works on; every GPU step under a time limit of its own (a
step that overruns ends the process with status 124, nothing is started after it).

    python tools/mutation_bench.py --config B --out profiles/mutation_bench.json   (N = 128, M = 10 000)
    python tools/mutation_bench.py --config C --out profiles/mutation_bench.json   (N = 500, M = 50 000)
Results of several configs are merged into one JSON file by config name."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libgdca.so: INTEGRATION.md "load order")

CONFIGS = {"B": dict(N=128, M=10000, theta=0.2, seed=0xB128), "C": dict(N=500, M=50000, theta=-1.0, seed=0xC500)}
KS = (1, 256, 8192)
PEAK_HBM = 8.0e12                  # bytes / s
FN_HBM_FRACTION = (0.58, 0.64)     # what k_fn20 reaches streaming the same matrix
CUS, GHZ, LDS_BYTES_PER_CLK = 256, 2.4, 128  # as the floors of sections 3.6 and 3.7 take the LDS of a compute unit


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("mutation_bench: step '%s' exceeded %d s\n" % (what, seconds))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutation_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, M, q, theta, pc = c["N"], c["M"], 21, c["theta"], args.pseudocount
    s = q - 1
    n = N * s
    DELTA, POTENTIAL = gd._lib.MUT_DELTA, gd._lib.MUT_POTENTIAL
    stream = torch.cuda.current_stream()
    with step_limit(60, "contexts"):
        ctx = gd.Context(0, stream=stream.cuda_stream)  # the torch stream: its events time the library's kernels
        torch.cuda.synchronize()
    Zo = synth_family(N, M, q, c["seed"])  # (M, N)
    KMAX = max(KS)
    with step_limit(60, "upload"):
        dZ = torch.from_numpy(Zo).cuda()
        dX = dZ[:KMAX].contiguous()  # N x K column-major: the first K sequences of the family
        dD = torch.empty(KMAX * N * q, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, M=M, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats, torch_repeats=args.torch_repeats,
               K={})

    # ---- the operator on a resident mJ (built by the library's own device operators)
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

    # ---- the route without this stage: gdca_energies_dev on the N q explicit mutants of one sequence (+ the wild type), scaled by K
    with step_limit(180, "explicit mutants"):
        x = dX[0]
        mut = x[None, :].repeat(N * q, 1)                                   # (N q, N): mutant i q + (b - 1)
        rows = torch.arange(N * q, device="cuda")
        mut[rows, rows // q] = (rows % q + 1).to(torch.int8)
        mut = torch.cat([mut, x[None, :]], dim=0).contiguous()
        dEm = torch.empty(N * q + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ms = timed(lambda: ctx.energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, mut.data_ptr(), N * q + 1, dEm.data_ptr()), args.warmup,
                   args.repeats)
        res["mutants_one_sequence_ms"] = statistics.median(ms)
        res["mutants_one_sequence_ms_all"] = ms
        res["mutants_note"] = "gdca_energies_dev on the N q mutants of ONE sequence and the sequence itself; the per-K figures are this " \
                              "time SCALED by K; building and uploading the mutants is not included"
        dE_mut = (dEm[:-1] - dEm[-1]).view(N, q)

    mJ = dmJ.view(n, n)
    for K in KS:
        r = {}
        with step_limit(240, "gdca_mutation_scan_dev K=%d" % K):
            for what, key in ((POTENTIAL, "operator_potential_ms"), (DELTA, "operator_ms")):
                ms = timed(lambda: ctx.mutation_scan_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dX.data_ptr(), K, what, dD.data_ptr()),
                           args.warmup, args.repeats)
                r[key] = statistics.median(ms)
                r[key + "_all"] = ms
            D_op = dD[:K * N * q].view(K, N, q).clone()
            torch.cuda.synchronize()
            scale = float(dE_mut.abs().max())
            r["mutants_vs_operator_max_abs_over_scale"] = float((D_op[0] - dE_mut).abs().max()) / scale
        with step_limit(300, "gdca_run_mutation_scan K=%d" % K):
            sts = []
            for i in range(args.warmup + args.repeats):
                st = ctx.run_mutation_scan_dev(dZ.data_ptr(), N, M, q, pc, theta, dX.data_ptr(), K, DELTA, dD.data_ptr())
                if i >= args.warmup:
                    sts.append(st)
            r["fused_ms_total"] = statistics.median(x_["ms_total"] for x_ in sts)
            r["fused_ms_score"] = statistics.median(x_["ms_score"] for x_ in sts)
            r["fused_ms_score_all"] = [x_["ms_score"] for x_ in sts]
            r["fused_vs_operator_max_abs_over_scale"] = float((dD[:K * N * q].view(K, N, q) - D_op).abs().max()) / float(D_op.abs().max())
        r["mutants_ms_scaled"] = res["mutants_one_sequence_ms"] * K

        # ---- floors.  HBM: the lower triangle once, X, the output, at k_fn20's fraction of the peak.  LDS: K N n lane reads of 8 bytes
        # (ds_read_b64, lane = row, the column wave-uniform: conflict-free), the LDS of a compute unit taken at 128 bytes a clock as in 3.6 / 3.7
        r["compulsory_bytes"] = 8.0 * n * (n + 1) / 2 + float(N) * K + 8.0 * q * N * K
        r["hbm_ms_at_fn_rate"] = [r["compulsory_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
        r["lds_bytes"] = 8.0 * K * N * n
        r["lds_ms_conflict_free"] = r["lds_bytes"] / (CUS * GHZ * 1e9 * LDS_BYTES_PER_CLK) * 1e3
        r["roofline_ms"] = max(min(r["hbm_ms_at_fn_rate"]), r["lds_ms_conflict_free"])
        r["roofline_fraction_operator_potential"] = r["roofline_ms"] / r["operator_potential_ms"]
        nR = -(-N // (64 // s))
        wide = -(-K // 128) * nR >= 2 * CUS
        r["matrix_passes"] = -(-K // (128 if wide else 16))  # every workgroup streams its 60 rows of the whole matrix (both triangles) itself
        r["tiling_bytes"] = r["matrix_passes"] * 8.0 * n * n + float(N) * K * 2 + 8.0 * q * N * K
        r["tiling_ms_at_fn_rate"] = [r["tiling_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]

        # ---- torch on the same GPU: symmetrise, encode, one dense matmul, the epilogue
        with step_limit(300, "torch formulation K=%d" % K):
            holder = {}

            def torch_scan():
                L = torch.tril(mJ)
                full = L + torch.tril(mJ, -1).t()
                Xk = dX[:K]
                Xl = Xk.long()
                oh = torch.zeros((K, n + 1), dtype=torch.float64, device="cuda")
                idx = torch.where(Xl < q, torch.arange(N, device="cuda")[None, :] * s + Xl - 1, torch.full_like(Xl, n))
                oh.scatter_(1, idx, 1.0)
                oh = oh[:, :n]
                g = full @ dPi
                F = (oh @ full).view(K, N, s)
                blocks = torch.diagonal(full.view(N, s, N, s), dim1=0, dim2=2).permute(2, 0, 1)  # [i, c, a] = mJ[r(i,c), r(i,a)]
                sym = torch.clamp(Xl - 1, max=s - 1)
                own = torch.gather(blocks[None].expand(K, N, s, s), 3, sym[:, :, None, None].expand(K, N, s, 1))[..., 0]
                own = torch.where((Xl < q)[:, :, None], own, torch.zeros_like(own))
                V = F - own + (0.5 * torch.diagonal(full) - g).view(1, N, s)
                V = torch.cat([V, torch.zeros((K, N, 1), dtype=torch.float64, device="cuda")], dim=2)
                holder["D"] = V - torch.gather(V, 2, (Xl - 1)[:, :, None])

            ms = timed(torch_scan, 1, args.torch_repeats)
            r["torch_ms"] = statistics.median(ms)
            r["torch_ms_all"] = ms
            r["torch_vs_operator_max_abs_over_scale"] = float((holder["D"] - D_op).abs().max()) / float(D_op.abs().max())
            holder.clear()
        r["speedup_vs_mutants_operator"] = r["mutants_ms_scaled"] / r["operator_ms"]
        r["speedup_vs_mutants_fused_stage"] = r["mutants_ms_scaled"] / r["fused_ms_score"]
        r["speedup_vs_torch_operator"] = r["torch_ms"] / r["operator_ms"]
        res["K"][str(K)] = r
        del D_op
    ctx.close()

    allres = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            allres = json.load(f)
    allres[args.config] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(allres, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
