// Where the three-plane bound of k_hamming stops carrying every pair of a tile (k_hamming.hip): the rule that picks the
// cut word from the probe's alive counts.  Plain C++ without a library call, so that k_hamming_decide (one device thread) and a host
// test (tests/test_hamming_cut_cpu.py compiles this header alone) run the very same arithmetic.
#pragma once

#if defined(__HIPCC__)
#define GDCA_CUT_HD __host__ __device__
#else
#define GDCA_CUT_HD
#endif

#define HAM_ALIVE_SLOTS 64    // sc->ham_alive[w - 1] = pairs of the sampled tiles still below the threshold after w words, w = 1 .. 64
#define HAM_LIST_WAVE 512     // entries of one wave's list of live pairs in LDS (four waves: 8 KB)
#define HAM_LIST_CAP (4 * HAM_LIST_WAVE)
#define HAM_CUT_MAX_NW 8000   // an entry's partial distance has 18 bits: 32 NW < 2^18

// The model, in units of one dense word of one thread (64 pairs x 4 instructions + the operands' LDS reads, ~277 wave instructions),
// with a = the alive fraction after w words and live = 16384 a = the entries of a tile's lists:
//   cost(w) = w                                           the dense words 0 .. w-1
//           + HAM_CUT_PASS0 + HAM_CUT_PASS1 * p_any(a)    the liveness pass: a compare and a branch per accumulator, and the
//                                                         append (8 instructions) where ANY of a wave's 64 lanes holds a live pair
//                                                         there, p_any = 1 - (1 - a)^64
//           + (NW - w) * (HAM_CUT_WORD + HAM_CUT_ENTRY * live / 256)   the sparse finish, lane = list entry: per remaining word the
//                                                         latency of one trip through the loop, and the entries' share of the LDS
// against cost = NW without a cut.  Instruction counts of the compiled kernel say PASS1 <= 1.85 and 0.1 per round of 256 entries and
// word; the constants below are fitted to the forced cuts measured on MI355X (profiles/hamming_cut_sweep.log: every HAM_CUT at
// configs B, C and D; overhead = words saved by the model's first term minus words saved on the clock).  Least squares over C and D:
// PASS0 = -0.15, PASS1 = 0.91, WORD = 0.067, ENTRY = 0.011, residuals below 0.12 words.  The pass and the sparse trips cost less than
// their instruction counts: the dense words saturate the vector ALUs, and a compare-and-branch pair or a trip of LDS reads mostly
// runs beside another wave's dense word.  PASS0 is negative because the form without a cut pays for its own last walk over the
// accumulators (the candidates), which the switch replaces.  Config B (four words, a tile bound by its fixed costs, where nothing
// hides the pass) puts the cut at word 2 BEHIND the one at word 3; PASS1 = 1.2 keeps that order as well as C's (12 before 13) and
// D's (24 before 25) and overstates the two largest overheads by 0.2 .. 0.35 words.
#define HAM_CUT_PASS0 -0.15
#define HAM_CUT_PASS1 1.2
#define HAM_CUT_WORD 0.07
#define HAM_CUT_ENTRY 0.011
#define HAM_CUT_MIN_GAIN 0.03  // no cut unless the model predicts at least this share of the kernel saved

// alive[w - 1], w = 1 .. min(NW, HAM_ALIVE_SLOTS): the probe's counts over `pairs` sampled pairs.  Returns the word at which the
// dense phase ends, 1 .. NW - 1, or NW = no cut.
static inline GDCA_CUT_HD int gdca_hamming_pick_cut(const unsigned *alive, double pairs, int NW)
{
    if (NW <= 2 || NW > HAM_ALIVE_SLOTS || !(pairs > 0.0)) return NW;
    int best = NW;
    double best_cost = (double)NW * (1.0 - HAM_CUT_MIN_GAIN);
    for (int w = 1; w < NW; ++w) {
        const double a = (double)alive[w - 1] / pairs;
        const double live = a * 16384.0;  // expected entries of a tile's list
        if (live > 0.5 * HAM_LIST_CAP) continue;
        double none = 1.0 - a;  // (1 - a)^64 by six squarings
        for (int i = 0; i < 6; ++i) none *= none;
        const double cost = (double)w + HAM_CUT_PASS0 + HAM_CUT_PASS1 * (1.0 - none) + (double)(NW - w) * (HAM_CUT_WORD + HAM_CUT_ENTRY * live / 256.0);
        if (cost < best_cost) {
            best_cost = cost;
            best = w;
        }
    }
    return best;
}
