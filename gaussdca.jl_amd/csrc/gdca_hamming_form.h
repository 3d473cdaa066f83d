// Which form counts the neighbours of a family (k_hamming.hip, k_hamming_fp4.hip): the rule k_hamming_decide applies to the
// probes' counts.  Plain C++ without a library call, so that the one device thread that decides and a host test
// (tests/test_hamming_form_cpu.py compiles this header alone) run the very same arithmetic.
//
//   0  exact       five planes, every pair of every tile to the end
//   1  three-plane the three low planes as a lower bound (dense to its cut word, then the pairs still alive), listed pairs refined
//   2  consensus   one plane -- "differs from the column's most frequent symbol" -- as a lower bound on the fp4 matrix pipe
//                  (k_hamming_fp4.hip), listed pairs refined
#pragma once

#if defined(__HIPCC__)
#define GDCA_FORM_HD __host__ __device__
#else
#define GDCA_FORM_HD
#endif

// The candidate list (k_hamming.hip: gdca_hamming_cand_cap) holds HAM_CAND_PER_TILE pairs per 128 x 128 tile of the triangle.  A bound
// form is only chosen where the probe says it fills at most HALF of that: the sample is 192 tiles, and a family clustered where
// the sample was not still fits.  (Overflow is never an error -- the exact form then counts the family -- only time lost.)
#define HAM_CAND_PER_TILE 64
#define HAM_FORM_MAX_DENSITY (0.5 * HAM_CAND_PER_TILE / 16384.0)  // 1.95e-3 of all pairs

// Between the exact and the three-plane form the rule is the one measured in round 3 and kept since: the bound below one candidate
// in a thousand pairs.
#define HAM_FORM_BOUND3_DENSITY 1e-3

// The consensus form against whichever of those two would run, by cost, in microseconds on MI355X:
//   three-plane   tiles x w_eff x HAM_T_DENSE + listed x (HAM_T_PAIR + N x HAM_T_REFINE),   w_eff = cut + HAM_CUT_TAIL (NW - cut) with
//                 the cut word k_hamming_decide has just picked (gdca_hamming_cut.h; no cut: w_eff = NW)
//   exact         tiles x NW x 1.5 HAM_T_DENSE                               (six instructions per word against four)
//   consensus     tiles x (HAM_T_TILE + E x HAM_T_ENTRY) + listed x (HAM_T_PAIR + N x HAM_T_REFINE) + M x E x HAM_T_IMAGE + HAM_T_FIXED
// tiles = the 128 x 128 tiles of the triangle, E = NW rounded up to the image's chunks of eight entries, listed = the probe's
// density x M^2 / 2.  The constants are fitted to the kernel times of forced forms at configs B, C, D and four families of E
// (profiles/consensus_bound_sweep.log: both forms' kernels traced per family):
//   three-plane loop, no cut   C 1.93e-3, D 1.76e-3, E 2.0 .. 2.5e-3 us per tile and word
//   product                    E = 8: 7.9e-3, E = 16: 8.6 .. 10.1e-3, E = 32: 12.3e-3 us per tile -- mostly per tile: the epilogue's
//                              scan was 61 % of a tile.  That scan has since been cut (C: 8.3e-3 -> 6.4e-3); the
//                              constants below are still this fit, which overstates the product and so chooses it later, never wrongly
//   refine                     0.86e-4 (N = 129) .. 1.1e-4 (N = 500) .. 2.3e-4 (N = 1000) us per listed pair
//   image                      0.9 .. 1.7e-5 us per row and entry, 4e-5 where N is not a multiple of four (bytes one by one)
#define HAM_T_DENSE 1.9e-3     // us per tile and word of the three-plane loop
#define HAM_CUT_TAIL 0.35      // what a word behind the cut still costs (C: cut 12 of 16 -> 0.84 of the dense time)
#define HAM_T_PAIR 0.7e-4      // us per listed pair of the refinement
#define HAM_T_REFINE 1.3e-7    // us per listed pair and position
#define HAM_T_TILE 6.5e-3      // us per tile of the fp4 product
#define HAM_T_ENTRY 1.6e-4     // us per tile and entry of the fp4 product
#define HAM_T_IMAGE 4.0e-5     // us per sequence and entry of the image
#define HAM_T_FIXED 25.0       // us: the histogram where theta is given, sigma, the probe, the empty grids of the forms not chosen

// Families below this many tile-words (~0.12 ms of three-plane loop) are not even probed for the consensus form: they would pay the
// histogram (theta given), the image and a probe for a product that can save a few tens of microseconds at the most.
#define HAM_FORM_MIN_WORK 65536.0

static inline GDCA_FORM_HD double gdca_hamming_tiles(int M)
{
    const double Mt = (double)((M + 127) / 128);
    return 0.5 * Mt * (Mt + 1.0);
}

// may the consensus form be chosen for an N x M family at all?  (host: decides what is allocated and launched)
static inline GDCA_FORM_HD int gdca_hamming_consensus_gate(int N, int M)
{
    const int NW = (N + 31) / 32;
    return NW > 2 && gdca_hamming_tiles(M) * (double)NW >= HAM_FORM_MIN_WORK;
}

// cand3 / cand1: pairs of the sampled tiles below the threshold under the three-plane / the consensus bound (cand1 < 0: that form
// was not probed); pairs: pairs sampled; cut: the three-plane form's cut word (>= NW: none).
static inline GDCA_FORM_HD int gdca_hamming_pick_form(double cand3, double cand1, double pairs, int N, int M, int cut)
{
    if (!(pairs > 0.0)) return 0;
    const int NW = (N + 31) / 32;
    const double tiles = gdca_hamming_tiles(M), all = 0.5 * (double)M * (double)M;
    const double f3 = cand3 / pairs, f1 = cand1 / pairs;
    const int other = f3 < HAM_FORM_BOUND3_DENSITY ? 1 : 0;
    if (cand1 < 0.0 || f1 > HAM_FORM_MAX_DENSITY) return other;
    const double weff = (cut > 0 && cut < NW) ? (double)cut + HAM_CUT_TAIL * (double)(NW - cut) : (double)NW;
    const double E = (double)((NW + 7) / 8 * 8), pair = HAM_T_PAIR + (double)N * HAM_T_REFINE;
    const double cost_other = other ? tiles * weff * HAM_T_DENSE + f3 * all * pair : tiles * (double)NW * 1.5 * HAM_T_DENSE;
    const double cost_cons = tiles * (HAM_T_TILE + E * HAM_T_ENTRY) + f1 * all * pair + (double)M * E * HAM_T_IMAGE + HAM_T_FIXED;
    return cost_cons < cost_other ? 2 : other;
}
