#!/usr/bin/env python3
"""Device time of the pair stage (k_pair_energy.hip) at two shapes: alone on a resident mJ (gdca_pair_energies_dev, energy and
coupling), as ms_score of the fused run (gdca_run_pair_energies_dev), against its LDS-gather and HBM floors, against the route the
library had before (gdca_energies_dev on the explicit concatenations a (+) b: timed on a 256 x 256 sub-block of the pairings and
SCALED by the pair count -- the full set would be K_A K_B N bytes), and against the obvious torch f64 formulation on the same GPU
(onehot(XA)' J_AB onehot(XB) plus the marginal quadratic forms).  One process; contexts are made before anything is timed; HIP events
on the stream the context works on; every GPU step under a time limit of its own (a step that overruns ends the process with status
124, nothing is started after it).

    python tools/pair_energy_bench.py --config B --out profiles/pair_energy_bench.json   (N = 128, split = 64, M = 10 000, K_A = K_B = 4096)
    python tools/pair_energy_bench.py --config C --out profiles/pair_energy_bench.json   (N = 500, split = 250, M = 50 000, K_A = K_B = 8192)
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

CONFIGS = {"B": dict(N=128, split=64, M=10000, K=4096, theta=0.2, seed=0xB128),
           "C": dict(N=500, split=250, M=50000, K=8192, theta=-1.0, seed=0xC500)}
PEAK_HBM = 8.0e12                  # bytes / s
FN_HBM_FRACTION = (0.58, 0.64)     # what k_fn20 reaches streaming the same matrix
CUS, GHZ, LDS_BYTES_PER_CLK = 256, 2.4, 128  # LDS bandwidth of a compute unit, bytes a clock (any read width, no bank conflict)
SUB = 256                          # the parent route is timed on SUB x SUB pairings


@contextlib.contextmanager
def step_limit(seconds, what):
    def over():
        sys.stderr.write("pair_energy_bench: step '%s' exceeded %d s\n" % (what, seconds))
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


def onehot(X, q):
    """(K, sites) symbols -> (K, sites * s) float64; the gap leaves its block zero"""
    K, S = X.shape
    s = q - 1
    out = torch.zeros((K, S * s + 1), dtype=torch.float64, device=X.device)
    Xl = X.long()
    idx = torch.where(Xl < q, torch.arange(S, device=X.device)[None, :] * s + Xl - 1, torch.full_like(Xl, S * s))
    out.scatter_(1, idx, 1.0)
    return out[:, :S * s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C", choices=sorted(CONFIGS))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--pseudocount", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_energy_bench.json"))
    args = ap.parse_args()
    assert args.repeats >= 10, "at least 10 timed repeats"

    import gaussdca.jl_amd as gd
    from gaussdca.jl_amd import devops
    from gaussdca.jl_amd.synth import synth_family

    c = CONFIGS[args.config]
    N, split, M, K, q, theta, pc = c["N"], c["split"], c["M"], c["K"], 21, c["theta"], args.pseudocount
    s = q - 1
    n, nA, nB, NA, NB = N * s, split * s, (N - split) * s, split, N - split
    ENERGY, COUPLING = gd._lib.PAIR_ENERGY, gd._lib.PAIR_COUPLING
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
        torch.cuda.synchronize()
    res = dict(config=args.config, N=N, split=split, M=M, KA=K, KB=K, q=q, n=n, theta=theta, pseudocount=pc, repeats=args.repeats,
               torch_repeats=args.torch_repeats)

    # ---- the fused run: ms_score is the pair stage
    with step_limit(240, "gdca_run_pair_energies"):
        sts = []
        for i in range(args.warmup + args.repeats):
            st = ctx.run_pair_energies_dev(dZ.data_ptr(), N, M, q, pc, theta, split, dXA.data_ptr(), K, dXB.data_ptr(), K, ENERGY, dE.data_ptr())
            if i >= args.warmup:
                sts.append(st)
        res["fused_ms_total"] = statistics.median(x["ms_total"] for x in sts)
        res["fused_ms_score"] = statistics.median(x["ms_score"] for x in sts)
        res["fused_ms_score_all"] = [x["ms_score"] for x in sts]
        E_fused = dE.clone()
        torch.cuda.synchronize()

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
    with step_limit(180, "gdca_pair_energies_dev"):
        for what, key in ((COUPLING, "operator_coupling_ms"), (ENERGY, "operator_ms")):
            ms = timed(lambda: ctx.pair_energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, split, dXA.data_ptr(), K, dXB.data_ptr(), K, what,
                                                     dE.data_ptr()), args.warmup, args.repeats)
            res[key] = statistics.median(ms)
            res[key + "_all"] = ms
        E_op = dE.clone()
        torch.cuda.synchronize()
        res["fused_vs_operator_max_rel"] = float(((E_fused - E_op).abs() / E_op.abs()).max())
        del E_fused

    # ---- the route without this stage: gdca_energies_dev on explicit concatenations, SUB x SUB pairings, scaled by the pair count
    with step_limit(180, "concatenation route"):
        a_idx = torch.arange(SUB, device="cuda").repeat(SUB)              # column a + SUB * b
        b_idx = torch.arange(SUB, device="cuda").repeat_interleave(SUB)
        dcat = torch.cat([dXA[a_idx], dXB[b_idx]], dim=1).contiguous()    # (SUB^2, N): N x SUB^2 column-major
        dEc = torch.empty(SUB * SUB, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ms = timed(lambda: ctx.energies_dev(dmJ.data_ptr(), dPi.data_ptr(), N, q, dcat.data_ptr(), SUB * SUB, dEc.data_ptr()), args.warmup,
                   args.repeats)
        res["concat_sub_pairs"] = SUB * SUB
        res["concat_sub_ms"] = statistics.median(ms)
        res["concat_ms_scaled"] = res["concat_sub_ms"] * (float(K) * K) / (SUB * SUB)
        res["concat_note"] = "gdca_energies_dev timed on %d x %d pairings and scaled by the pair count; building and uploading the " \
                             "concatenations is not included" % (SUB, SUB)
        sub = E_op.view(K, K)[:SUB, :SUB].reshape(-1)  # E_op is column-major: view(K, K)[b, a] -> entry a + SUB * b
        res["concat_vs_operator_max_rel"] = float(((dEc - sub).abs() / sub.abs()).max())
        del dcat, dEc

    # ---- floors of the pair stage.  The LDS model: the LDS of a compute unit delivers 128 bytes a clock whatever the width of the
    # read, and NO bank conflict is assumed.  The fold reads K_A N_A n_B doubles (ds_read_b64, lane = row: really conflict-free);
    # the gather reads K_A K_B N_B doubles as 64-byte rows (four ds_read_b128 a symbol for eight pairings) at per-lane random rows,
    # where conflicts are likely: the figure is a lower bound of the time, not a model of the access pattern.
    lds_bytes = 8.0 * (float(K) * NA * nB + float(K) * K * NB)
    res["lds_bytes"] = lds_bytes
    res["lds_bytes_per_clk_per_cu"] = LDS_BYTES_PER_CLK
    res["lds_ms_conflict_free"] = lds_bytes / (CUS * GHZ * 1e9 * LDS_BYTES_PER_CLK) * 1e3
    res["compulsory_bytes"] = 8.0 * nA * nB + 8.0 * K * K + float(N) * K * 2
    res["hbm_ms_at_fn_rate"] = [res["compulsory_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    wide = -(-K // 128) * -(-nB // 64) >= 2 * CUS
    res["fold_block_passes"] = -(-K // (128 if wide else 16))      # every fold workgroup row streams its 64 rows of the block itself
    res["tiling_bytes"] = res["fold_block_passes"] * 8.0 * nA * nB + 2 * 8.0 * K * nB + 8.0 * K * K
    res["tiling_ms_at_fn_rate"] = [res["tiling_bytes"] / (f * PEAK_HBM) * 1e3 for f in FN_HBM_FRACTION]
    roof = max(min(res["hbm_ms_at_fn_rate"]), res["lds_ms_conflict_free"])
    res["roofline_ms"] = roof
    res["roofline_fraction_operator_coupling"] = roof / res["operator_coupling_ms"]

    # ---- the same matrix by torch on the same GPU
    with step_limit(600, "torch formulation"):
        mJ = dmJ.view(n, n)
        J_AB = mJ[nA:, :nA]                                         # rows of B, columns of A (mJ is symmetric)
        holder = {}

        def torch_coupling():
            holder["R"] = (onehot(dXA, q) @ J_AB.t()) @ onehot(dXB, q).t()

        def torch_energy():
            oa, ob = onehot(dXA, q), onehot(dXB, q)
            R = (oa @ J_AB.t()) @ ob.t()
            g = mJ @ dPi
            c0 = dPi @ g
            # E(a (+) gaps) = 1/2 a' J_AA a - a' g_A + c0 / 2, likewise b
            ea = 0.5 * ((oa @ mJ[:nA, :nA]) * oa).sum(dim=1) - oa @ g[:nA] + 0.5 * c0
            eb = 0.5 * ((ob @ mJ[nA:, nA:]) * ob).sum(dim=1) - ob @ g[nA:] + 0.5 * c0
            holder["E"] = ea[:, None] + eb[None, :] - 0.5 * c0 + R

        ms = timed(torch_coupling, 1, args.torch_repeats)
        res["torch_coupling_ms"] = statistics.median(ms)
        res["torch_coupling_ms_all"] = ms
        holder.pop("R")
        ms = timed(torch_energy, 1, args.torch_repeats)
        res["torch_ms"] = statistics.median(ms)
        res["torch_ms_all"] = ms
        Eo = E_op.view(K, K).t()  # [a, b]
        res["torch_vs_operator_max_rel"] = float(((holder["E"] - Eo).abs() / Eo.abs()).max())
    res["speedup_vs_concat_operator"] = res["concat_ms_scaled"] / res["operator_ms"]
    res["speedup_vs_concat_fused_stage"] = res["concat_ms_scaled"] / res["fused_ms_score"]
    res["speedup_vs_torch_operator"] = res["torch_ms"] / res["operator_ms"]
    res["speedup_vs_torch_fused_stage"] = res["torch_ms"] / res["fused_ms_score"]
    res["speedup_vs_torch_coupling"] = res["torch_coupling_ms"] / res["operator_coupling_ms"]
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
