// igemm16_plan.hip - the launch plans of the bf16-resident kernels: every predicate that decides which kernel of
// igemm16.hip a launch takes and how (igemm16_plan.h).  Host only.
#include "igemm16_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" char** environ;

namespace bg {

static int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

// The per-call switches in ONE pass over the environment (about the cost of a single getenv).
Tune16 tune16() {
    static const Tune16 once = {env_int("BG_NN16_SLOTS", 512), env_int("BG_NN16_HALO_CMAX", 4096),  // (the first six fields)
                                env_int("BG_TN16_WANT", 1024), env_int("BG_TN16_WIDE", 1),
                                env_int("BG_TN16X_WANT", 512), env_int("BG_TN16X_BK", 32)};
    Tune16 t = once;
    t.posmajor = t.halo = t.thin_d2s = t.tn16x_nbi = 1;
    t.tn16x_phased = -1;
    t.tn16x_phased_ring = 6;
    for (char** e = environ; e && *e; ++e) {
        const char* s = *e;
        if (s[0] != 'B' || s[1] != 'G' || s[2] != '_') continue;
        const char* v = strchr(s, '=');
        if (!v) continue;
        const size_t n = v++ - s;
        auto is = [&](const char* name) { return strlen(name) == n && memcmp(s, name, n) == 0; };
        if (is("BG_NN16_POSMAJOR")) t.posmajor = atoi(v) != 0;
        else if (is("BG_NN16_PIPE")) t.pipe_set = 1, t.pipe = atoi(v);
        else if (is("BG_NN16X_BN")) t.nn16x_bn = atoi(v);
        else if (is("BG_NN16_HALO")) t.halo = atoi(v);
        else if (is("BG_NN16_HALO_K3S2")) t.halo_k3s2 = atoi(v) == 1;
        else if (is("BG_THIN_D2S")) t.thin_d2s = atoi(v);
        else if (is("BG_NN16_MFAST")) t.mfast = strcmp(v, "auto") == 0 ? 2 : atoi(v) != 0;
        else if (is("BG_TN16X_NBI")) t.tn16x_nbi = atoi(v) == 2 ? 2 : 1;
        else if (is("BG_TN16X_PHASED")) t.tn16x_phased = atoi(v) != 0;
        else if (is("BG_TN16X_PHASED_BN")) t.tn16x_phased_bn = atoi(v);
        else if (is("BG_TN16X_PHASED_RING")) t.tn16x_phased_ring = atoi(v);
    }
    return t;
}

struct NN16Plan { int tn, splitk; };

static int nn16_steps_min(const NN16Params& p, int mode) {
    int per_axis = p.g.k;
    if (mode == GATHER_TCONV && p.g.pstep > 1) per_axis = max(1, p.g.k / p.g.stride);
    return (per_axis * per_axis * (p.C >> 3) + 7) >> 3;
}

// Fraction of the (row, tap) pairs of a launch that have a source pixel: 1 for reflect-padded forward gathers, 16 / 36
// for the input gradient of a 3 x 3 convolution on the padded 6 x 6 grid of a 4 x 4 map.  Separable per axis.
static double nn16_axis_fraction(const Gather& g, int mode, int nq, int n_src) {
    int64_t valid = 0, slots = 0;
    for (int ph = 0; ph < (mode == GATHER_TCONV ? g.pstep : 1); ++ph) {
        int k0 = 0, kstep = 1, nk = g.k;
        if (mode == GATHER_TCONV && g.pstep > 1) {
            kstep = g.stride;
            k0 = (ph + g.pad) % g.stride;
            nk = (g.k - k0 + g.stride - 1) / g.stride;
        }
        for (int q = 0; q < nq; ++q) {
            const int o = q * g.pstep + ph;
            for (int i = 0; i < nk; ++i) {
                const int kk = k0 + i * kstep;
                bool ok;
                if (mode == GATHER_CONV) {
                    const int src = o * g.stride + kk - g.pad;
                    ok = g.reflect || (src >= 0 && src < n_src);
                } else {
                    const int hn = o + g.pad - kk;
                    ok = hn >= 0 && hn % g.stride == 0 && hn / g.stride < n_src;
                }
                valid += ok;
            }
            slots += nk;
        }
    }
    return slots ? (double)valid / (double)slots : 1.0;
}

// Position-major rows (NN16Params::posmajor) when at least a tenth of the tap walk would run on the zero page and a
// 128-row tile covers few positions (BG_NN16_POSMAJOR=0 switches it off; read per call so that a test can compare).
static double nn16_posmajor_fraction(const Tune16& t, const NN16Params& p, int mode) {
    if (!t.posmajor) return 1.0;
    const Gather& g = p.g;
    if (g.k <= 1 || g.Nb < 16 || g.Hq <= 0 || g.Wq <= 0 || (int64_t)g.Hq * g.Wq > 40 * 40) return 1.0;
    const double f = nn16_axis_fraction(g, mode, g.Hq, g.Hs) * nn16_axis_fraction(g, mode, g.Wq, g.Ws);
    return f < 0.9 ? f : 1.0;
}

// Tile width and split-K by a round model: the grid runs in rounds of `slots` co-resident blocks (2 per CU); a block's
// time is its K steps x (A-side work + one unit per 32 output columns).  Fewer, wider tiles waste padded columns and
// can leave the last round (or the only one) mostly empty; narrow ones re-read the A tile more often.
//   pm: nn16_posmajor_fraction of the launch
static NN16Plan plan_nn16(const Tune16& t, const NN16Params& p, int mode, int zdim, double pm, bool allow_split) {
    const int slots = t.nn16_slots;
    const int64_t tm = (p.M + P16_BM - 1) / P16_BM;
    int steps = nn16_steps_min(p, mode);
    if (pm < 1.0) steps = max(1, (int)(steps * pm + 0.5));       // taps without sources are not walked
    NN16Plan best{4, 1};
    double best_cost = 1e30;
    for (int tn = 4; tn >= 1; --tn) {
        const int bn = 32 * tn;
        const int64_t tiles = tm * ((p.N + bn - 1) / bn) * zdim;
        const double unit = 1.5 + tn;
        const int max_sk = allow_split ? (steps / 4 < 16 ? (steps / 4 < 1 ? 1 : steps / 4) : 16) : 1;
        for (int sk = 1; sk <= max_sk; ++sk) {
            const int64_t rounds = (tiles * sk + slots - 1) / slots;
            double cost = (double)rounds * ((steps + sk - 1) / sk + 2.0) * unit;     // + prologue / epilogue per block
            if (sk > 1) cost += 6.0 * unit + 0.02 * sk * (double)tiles / slots * bn; // reduce launch + slab traffic
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best = NN16Plan{tn, sk};
            }
        }
    }
    return best;
}

// Which pipeline form of nn16_kernel a launch takes (see the kernel's header).  The forms give bit-identical results, so
// this is a matter of speed alone; the plan (tile width, split-K) does not depend on it.
//   tn: the plan's tile width; row_blocks: 256-row tiles x stride phases x K splits of the launch; even_phases: every
//   stride phase walks the same number of taps; mirrored: a mirrored-tap launch (NN16Params::ring), which has no 8-wave
//   instantiation; *xtn: the phased form's own column tile BN / 32 (the plan's tn is for the 128-row tile).
// BG_NN16_PIPE (read per call: tests/test_gpu_nn16_pipe.py and test_gpu_nn16_phased.py compare the forms) = 0: two stages
// everywhere, 1: the ring form at the 128-row block wherever it applies, 2: the wide form wherever it applies, 3: the phased
// form wherever it applies; unset: the rule below.  BG_NN16X_BN = 128 | 192 | 256 (read per call; the tests and
// tools/kbench.py only) overrides the phased form's column tile.
//
// The rule, from the per-layer tables of profiles/nn16_pipe_ab.txt (config 3 at 256 and at 32 images, forward / input
// gradient, ms, two stages -> wide form):
//   C <= 192 per tap, image-major rows, a grid of at least one round of blocks (2 per CU) - the wide form:
//       conv 96 -> 192 k3 s2 at 64^2 0.33 / 0.45 -> 0.27 / 0.39, 192 -> 384 k3 s2 at 32^2 0.20 / 0.27 -> 0.18 / 0.25, input
//       gradients of the k4 s2 transposed convs 192 -> 96 at 64^2 0.93 -> 0.81 and 384 -> 192 at 32^2 0.65 -> 0.62, the 1 x 1
//       convs 192 -> 96 0.14 / 0.23 -> 0.13 / 0.19, 96 -> 192 0.22 / 0.14 -> 0.19 / 0.13, 192 -> 24 input gradient 0.20 -> 0.14.
//       These layers re-read activations, not weights: the 256-row tile halves the weight-tile traffic per row and its
//       ring keeps two tiles in flight per block.
//   32-column tiles (192 -> 24 forward: 0.091 -> 0.097), the ring forms at C >= 384 (within +-0.01 of the two-stage form at
//       256 images, up to 20 % slower at 32, where the 256-row grid falls under one round) and position-major rows: two stages.
//   C >= 384 per tap, image-major rows or position-major rows with Nb % 256 == 0, a grid of WHOLE rounds of one block per CU -
//       the phased form (profiles/nn16x_phase_ab.txt; config 3 at 256 images, ms per call, two stages -> BN 128 / 192 / 256,
//       forward ; input gradient; blocks at BN 128 / 192 / 256):
//         deconv 4^2 1536 -> 1536 k4 s2    0.341 -> 0.318 / 0.300 / 0.333 ; 0.348 -> 0.333 / 0.318 / 0.343   (768 / 512 / 384)
//         deconv 8^2 1536 -> 1536 k3       0.617 -> 0.627 / 0.566 / 0.678 ; 0.605 -> 0.600 / 0.548 / 0.651   (768 / 512 / 384)
//         deconv 8^2 1536 -> 768 k4 s2     0.639 -> 0.559 / 0.493 / 0.466 (1536 / 1024 / 768) ; 0.539 -> 0.531 / 0.482 / 0.574
//         deconv 16^2 768 -> 384 k4 s2     (forward: halo kernel) ; 0.586 -> 0.607 / 0.559 / 0.515   (1536 / 1024 / 768)
//         deconv 32^2 384 -> 192 k4 s2     (forward: halo kernel) ; 0.644 -> 0.660 / 0.583 / 0.702   (3072 / 2048 / 2048)
//         conv 16^2 384 -> 768 k3 s2       0.159 -> 0.170 / 0.152 / 0.176 ; 0.224 -> 0.243 / 0.218 / 0.246
//         conv 8^2 768 -> 768 k3           0.298 -> 0.311 / 0.275 / 0.329 ; 0.408 -> 0.419 / 0.384 / 0.441   (768 / 512 / 384)
//         conv 8^2 768 -> 1536 k3 s2       0.186 -> 0.193 / 0.178 / 0.208 ; 0.260 -> 0.261 / 0.248 / 0.255
//         conv 4^2 1536 -> 1536 k3         0.323 -> 0.334 / 0.298 / 0.350 ; 0.552 -> 0.552 / 0.534 / 0.560   (768 / 512 / 384)
//       (repeat spread of a layer: 0.001 - 0.006).  The form runs ONE block per CU, so what decides is whether the grid comes
//       out in whole rounds of 256 blocks: BN = 256 wins only where it does (768 blocks: 1330 TF/s on 1536 -> 768 k4 s2) and
//       loses at 384 blocks = 1.5 rounds; BN = 128 fills the rounds but fetches 3/4 of the two-stage form's L2 -> LDS bytes
//       per FLOP and ties it.  1536, 768 and 384 output channels are whole multiples of 192, and 192-column tiles bring every
//       one of these launches to 512, 1024 or 2048 blocks.  Hence: BN = 256 when N % 256 == 0, the grid is whole rounds at
//       256 columns and the stride phases are even (k3 s2 phases walk 1 / 2 / 2 / 4 taps: 768 -> 1536 k3 s2 input gradient,
//       1536 blocks at BN 256, is slower there than at 192); otherwise BN = 192 when 192-column tiles pad N to no more columns
//       than the plan's own tiles do (N % 192 == 0 here; at N = 256, 512 or 1024 they would add 12 - 50 % of MFMA work, at
//       N <= 64 many times the plan's - none of those measured, all left on two stages), the grid leaves at most 1/16 of the
//       256 slots of its last round empty, however many rounds there are (a round half empty costs BN = 256 the 8 - 10 %
//       the form gains) and, with uneven phases, has at least two rounds (768 -> 1536 k3 s2 input gradient at 256 images, ONE round of 256 blocks: 0.195 -> 0.215 per call in the
//       step, the CUs that drew a 1-tap phase idle while the 4-tap blocks finish; at 512 images, two rounds, 0.259 -> 0.251);
//       otherwise two stages.  At 32 images the rule leaves most of these launches on two stages and every C >= 384 layer is
//       within the repeat spread (0.002 - 0.008 ms) of BG_NN16_PIPE=0.  Grids of partly filled rounds other than the 1.5
//       above: not measured.
//   The ring at the 128-row block is the default nowhere: where it gains (the C <= 192 layers above) the wide form gains
//       more, and on the C >= 768 maps of 4^2 ... 8^2 it LOSES 25 - 40 % (1536 -> 1536 k3 at 8^2: 0.62 -> 0.87): those launches
//       stream 10 - 40 MB of weights through L2 and a 32-channel stage reads only half of every 128-byte line per
//       LDS-DMA, so each line is requested twice, one step apart - with three blocks per CU streaming 48 KB per step
//       through the CU's 32 KB vector cache in between.  It stays behind the switch for the comparison.
constexpr int NN16X_CUS = 256;                // one phased block per CU (plan_nn16 counts 512 slots of two blocks per CU)
static int nn16_form(const Tune16& t, const NN16Params& p, bool posmajor, int tn, int64_t row_blocks, bool even_phases,
                     bool mirrored, int* xtn) {
    // The 256-row forms on position-major rows: a position-major tile walks the taps that ITS rows have sources under, so a
    // 256-row tile would walk other taps (and split K elsewhere) than the two 128-row tiles it replaces - other sums -
    // unless it lies inside one position, as both of those tiles then do: Nb % 256 == 0.  The wide form has no
    // position-major instantiation at all.
    const bool wide_ok = !mirrored && !posmajor && p.g.Ws < (1 << 15);   // (the ring forms keep source columns as int16)
    const bool phased_ok = !mirrored && (!posmajor || p.g.Nb % 256 == 0);
    const int64_t wide_blocks = row_blocks * ((p.N + 32 * tn - 1) / (32 * tn));
    // BN of the phased form by the rule (0: the rule leaves the launch on two stages)
    const int64_t nb256 = row_blocks * ((p.N + 255) / 256), nb192 = row_blocks * ((p.N + 191) / 192);
    const int64_t last192 = (nb192 + NN16X_CUS - 1) / NN16X_CUS * NN16X_CUS - nb192;      // empty slots of the last round
    // columns the 192-wide tiles pad N to, against the plan's own tiles: never more MFMA work than the plan's
    const int pad192 = (p.N + 191) / 192 * 192, pad_plan = (p.N + 32 * tn - 1) / (32 * tn) * (32 * tn);
    int bn = 0;
    if (phased_ok && p.C >= 384) {
        if (p.N % 256 == 0 && nb256 % NN16X_CUS == 0 && even_phases) bn = 256;
        else if (pad192 <= pad_plan && nb192 >= (even_phases ? 1 : 2) * NN16X_CUS && last192 * 16 <= NN16X_CUS) bn = 192;
    }
    const int rule_bn = bn;
    if (bn == 0) bn = p.N <= 128 ? 128 : (p.N <= 192 ? 192 : 256);       // (forced by the switch)
    if (t.nn16x_bn == 128 || t.nn16x_bn == 192 || t.nn16x_bn == 256) bn = t.nn16x_bn;
    *xtn = bn / 32;
    if (t.pipe_set) {
        const int v = t.pipe;
        if (v == 3) return phased_ok ? NN16_FORM_PHASED : NN16_FORM_TWO;
        if (v == 2) return wide_ok ? NN16_FORM_WIDE : NN16_FORM_TWO;
        return (v == 1 && p.g.Ws < (1 << 15)) ? NN16_FORM_RING : NN16_FORM_TWO;
    }
    if (rule_bn) return NN16_FORM_PHASED;
    return (wide_ok && p.C <= 192 && tn >= 2 && wide_blocks >= 512) ? NN16_FORM_WIDE : NN16_FORM_TWO;
}

static int nn16h_taps(const Tune16& t, const NN16Params& p, int mode, int zdim) {
    // On by default (BG_NN16_HALO=0 switches it off; read per call so that a test can compare both forms).  Measured r02,
    // config 3 at batch 256: forward sum over the 22 layer shapes 10.62 -> 9.18 ms, input gradients 12.31 -> 11.65 ms;
    // transposed conv 96 -> 96 at 128^2: 600 -> 825 TF/s, 768 -> 768 at 16^2: 1083 -> 1198 (forward), 1276 (input gradient).
    const int use = t.halo, cmax = t.halo_cmax;
    const Gather& g = p.g;
    constexpr int T = P16_HALO_T;
    if (!use || p.C > cmax || p.C % 32 || p.N % 8 || g.Hq < T || g.Wq < T || g.Hq % T || g.Wq % T) return 0;
    if (mode == GATHER_CONV) return (g.stride == 1 && g.k == 3 && g.pstep == 1 && zdim == 1) ? 3 : 0;
    if (g.reflect) return 0;
    if (g.stride == 1 && g.k == 3 && g.pstep == 1 && zdim == 1) return 3;
    if (g.stride == 2 && g.k == 4 && g.pstep == 2 && zdim == 4) return 2;
    // r03: the stride phases of a 3 x 3 stride-2 transposed gather (input gradients of the discriminator's down-sampling
    // convolutions): windows of 1 x 1, 1 x 2, 2 x 1 and 2 x 2 taps inside the 2 x 2 halo.  OFF by default (BG_NN16_HALO_K3S2=1
    // turns it on): measured on config 3 at batch 256, tap kernel -> this form: 64^2 96 <- 192: 0.435 -> 0.402 ms per call,
    // 32^2 192 <- 384: 0.29 -> 0.37 - a block of the 1-tap phase loads a 17 x 17 halo and stores a full patch for a
    // quarter of the MFMA work, so the halo's saving in L2 -> LDS bytes does not pay.
    if (g.stride == 2 && g.k == 3 && g.pad == 1 && g.pstep == 2 && zdim == 4) return t.halo_k3s2 ? 2 : 0;
    return 0;
}

// The THIN = 1 form of nn16h_kernel (see there): p describes the plain transposed gather (A = dy [Nb, Hs, Ws, C], B = the
// packed [9][8][C] kernel, out = dx [Nb, 2 Hs, 2 Ws, 8]).
bool nn16h_d2s_ok(const Tune16& t, const NN16Params& p) {
    const int use = t.thin_d2s;                         // (read per call: a test compares both forms)
    const Gather& g = p.g;
    return use && p.N == 8 && p.out_ld == 8 && g.k == 3 && g.stride == 2 && g.pad == 1 && !g.reflect && p.C % 32 == 0 &&
           g.Hs % P16_HALO_T == 0 && g.Ws % P16_HALO_T == 0 && g.Ho == 2 * g.Hs && g.Wo == 2 * g.Ws && !p.bias && !p.stats_part;
}

// Which operand should stay in an XCD's L2 (4 MB) while the other streams: estimated fabric bytes of the two tile orders.
// OFF by default: measured r03 (config 3, batch 256, same box): N-tiles fastest 100.9 ms / iteration, this rule 102.0, M-tiles
// fastest everywhere 103.7 - the weight slabs the N-fastest order re-fetches once per M-tile (round 2's FETCH_SIZE counters:
// 1.9 GB per launch on the 4 x 4 ... 16 x 16 layers) come out of the 256 MB Infinity Cache, not out of HBM, and cost no time,
// while M-fastest makes every co-resident block miss on its own gathered rows.  BG_NN16_MFAST=auto applies the rule, =1
// forces M-fastest (for counter runs).
static int nn16_mfast(const Tune16& t, const NN16Params& p, int tiles_m, int tiles_n) {
    if (t.mfast != 2) return t.mfast;
    const double l2 = 3.0e6;
    const double a_bytes = 2.0 * p.g.Nb * (double)p.g.Hs * p.g.Ws * p.g.ld;
    const double w_bytes = 2.0 * p.g.k * p.g.k * (double)p.N * p.C;
    const double nfast = a_bytes + (w_bytes > l2 ? w_bytes * tiles_m : w_bytes);
    const double mfast = w_bytes + (a_bytes > l2 ? a_bytes * tiles_n : a_bytes);
    return mfast < nfast;
}

// Column tile / 32 of the halo-tile kernel (NF) and of the mirrored-tap launch:
static int least_padded_tile(int N) {
    int nf = 4, best = 1 << 30;
    // (c = 1, a 32-column tile, r03: the generator's 96 -> 3 (8) image layer - a quarter of the padded MFMA work of the
    //  64-column tile and the input read once instead of once per tap by the tap kernel)
    // Least padded output channels; ties: the wider tile.  N = 384 / 768 pad alike at 128 and 96 columns; measured on
    // config 3 at batch 256 (profiles/halo_ring_ab.txt; NF = 4 against NF = 3, forward / input gradient, ms):
    // 16^2 768 -> 384 k4s2 0.53 against 0.59, 32^2 384 -> 384 k3 0.55 / 0.55 against 0.61 / 0.60, 16^2 768 -> 768 k3 0.53 / 0.53
    // against 0.58 / 0.56 - the narrower tile loads the halo 4/3 times as often.
    for (int c = 4; c >= 1; --c) {
        const int padded = (N + 32 * c - 1) / (32 * c) * (32 * c);
        if (padded < best) { best = padded; nf = c; }
    }
    return nf;
}

static void plan_tn16(const Tune16& t, const TN16Params& p, int* sk_out, int* rps_out) {
    const int64_t tiles = (int64_t)((p.Mf + 127) / 128) * ((p.Cb + 127) / 128);
    const int want = t.tn16_want;
    int sk = (int)(want / tiles);          // (floor: tiles * sk <= want = a whole number of rounds of 512 co-resident blocks)
    const int max_sk = (p.M + 4 * P16_TN_BK - 1) / (4 * P16_TN_BK);      // at least 256 pixels per split
    if (sk > max_sk) sk = max_sk;
    if (sk < 1) sk = 1;
    if (sk > 512) sk = 512;
    int rps = (p.M + sk - 1) / sk;
    rps = (rps + P16_TN_BK - 1) / P16_TN_BK * P16_TN_BK;
    *sk_out = (p.M + rps - 1) / rps;
    *rps_out = rps;
}

// wide form (tn16x_kernel): used when there are at least two 128-row tiles of output and the reduction fills the ring;
// split so that the grid is a whole number of rounds of 256 co-resident blocks (one per CU)
// 256-wide output tiles (tn16x_kernel<.., 2>) where they divide the output channels: C = 512, 768, 1536.  OFF by default:
// measured r03 (config 3, same box): 102.7 ms / iteration with it, 102.9 without at batch 256, 25.6 / 25.6 at batch 32 -
// the third fewer L2 -> LDS bytes and LDS operand reads buy nothing once only one block (2 waves per SIMD) fits a CU.
// BG_TN16X_NBI=2 switches it on (tests/test_gpu_bf16.py keeps it exact).
static int tn16x_nbi(const Tune16& t, const TN16Params& p) {
    if (t.tn16x_nbi != 2) return 1;
    return (p.Cb >= 512 && p.Cb % 256 == 0 && p.Mf >= 256) ? 2 : 1;
}

// Column tile of the phased form (tn16x_phased_kernel) for a launch that plan_tn16x accepts; 0: the launch keeps
// tn16x_kernel<.., 32>.  The K partition is plan_tn16x's for 128-column tiles whatever the tile (same sums, same workspace):
// tm: 256-row tiles, sk: K splits of that plan, so the phased grid is tm * ceil(Cb / BN) * sk blocks.
// Switches, read per call (tests/test_gpu_tn16x_phased.py, tools/kbench.py): BG_TN16X_PHASED = 0: never, 1: every launch
// the wide form accepts (gathered operands only: the regulariser's Gram keeps the ring form - not measured); unset: the
// rule.  BG_TN16X_PHASED_BN = 192 / 256 sets the column tile of a launch that takes the form.  With BG_TN16X_NBI=2 set, the
// launches that switch applies to go where it sends them.  (BG_TN16X_PHASED_RING=8: the 128 KB ring, for A/B.)
//
// The rule, from the per-layer table of profiles/tn16x_phase_ab.txt (config 3 at 256 images, tools/kbench.py wgrad column,
// ms per call: tn16x_kernel<0, 32> -> BN 192 / BN 256 ; Cb ; blocks at 128 / 192 / 256 columns; repeat spread 0.001 - 0.010):
//   deconv 64^2 192 -> 96 k4 s2      0.889 -> 0.694 / 0.780   Cb  192   504 / 252 / 252
//   deconv 64^2 192 -> 192 k3        0.976 -> 0.781 / 0.870   Cb  192   504 / 252 / 252
//   conv 64^2 96 -> 192 k3 s2        0.290 -> 0.221 / 0.246   Cb  192   512 / 256 / 256
//   conv 32^2 192 -> 192 k3          0.502 -> 0.385 / 0.419   Cb  192   504 / 252 / 252
//   deconv 32^2 384 -> 192 k4 s2     0.693 -> 0.866 / 0.952   Cb  384   504 / 336 / 336
//   deconv 32^2 384 -> 384 k3        0.769 -> 1.000 / 1.163   Cb  384   504 / 336 / 336
//   conv 32^2 192 -> 384 k3 s2       0.210 -> 0.283 / 0.307   Cb  384   504 / 336 / 336
//   conv 16^2 384 -> 384 k3          0.359 -> 0.506 / 0.566   Cb  384   504 / 336 / 336
//   deconv 16^2 768 -> 384 k4 s2     0.742 -> 0.994 / 0.635   Cb  768   432 / 288 / 216
//   deconv 16^2 768 -> 768 k3        0.684 -> 0.989 / 0.588   Cb  768   486 / 324 / 243
//   conv 16^2 384 -> 768 k3 s2       0.205 -> 0.279 / 0.184   Cb  768   504 / 336 / 252
//   conv 8^2 768 -> 768 k3           0.385 -> 0.525 / 0.349   Cb  768   486 / 324 / 243
//   deconv 8^2 1536 -> 768 k4 s2     0.777 -> 0.749 / 0.802   Cb 1536   576 / 384 / 288
//   deconv 8^2 1536 -> 1536 k3       0.821 -> 0.796 / 0.842   Cb 1536   648 / 432 / 324
//   deconv 4^2 1536 -> 1536 k4 s2    0.370 -> 0.338 / 0.355   Cb 1536  1152 / 768 / 576
//   conv 8^2 768 -> 1536 k3 s2       0.259 -> 0.195 / 0.224   Cb 1536   324 / 216 / 162
//   conv 4^2 1536 -> 1536 k3         0.414 -> 0.401 / 0.446   Cb 1536   648 / 432 / 324
//   (forced onto Cb = 96 and 24 the form loses 8 - 60 %: one partly filled tile.)
// The form runs ONE block per CU under a split that was planned for 512 slots of 128 columns, and the split stays (the sums
// depend on it).  What decides is therefore how the grid falls into rounds of 256 blocks.  With whole 192-column tiles the
// Cb = 192 layers come out at 252 - 256 blocks without the parent's half-empty second tile (-20 ... -24 %), 768 -> 1536 k3 s2
// at 216 (-25 %) and 1536 -> 1536 k4 s2 at three whole rounds (-9 %).  At Cb = 768 three 256-column tiles make 216 - 252
// blocks (-9 ... -14 %) where four 192-column tiles make 1.1 - 1.3 rounds (+35 ... 45 %).  Cb = 384 has no tile that fills
// its rounds (336 blocks: +25 ... 40 %).  The Cb = 1536 launches of 1.5 - 1.7 rounds gain 3 - 4 % at 192 (their parent grids,
// 576 - 648 blocks on 512 slots, do not fill their rounds either) and lose at 256.  Hence: BN = 192 where Cb % 192 == 0,
// else BN = 256 where Cb % 256 == 0, each only if the last round of its grid is at least half full (measured: 0 - 128 empty
// slots gain, 176 and more lose; grids under half a round and Cb % 256 == 0 with Cb % 192 != 0: not measured) - otherwise the
// parent form: Cb = 96, 24, 8, every tail, every grid that does not fill its rounds.
constexpr int TN16XP_CUS = 256;
static int tn16x_phased_bn(const Tune16& t, const TN16Params& p, int mode, int nbi, int tm, int sk) {
    if (mode != GATHER_CONV || nbi != 1) return 0;
    int bn = 0;
    for (int c = 192; c <= 256 && bn == 0; c += 64) {
        const int64_t blocks = (int64_t)tm * (p.Cb / c) * sk;
        const int64_t last = (blocks + TN16XP_CUS - 1) / TN16XP_CUS * TN16XP_CUS - blocks;      // empty slots of the last round
        if (p.Cb % c == 0 && last * 2 <= TN16XP_CUS) bn = c;
    }
    if (t.tn16x_phased >= 0) {
        if (t.tn16x_phased == 0) return 0;
        if (bn == 0) bn = (p.Cb > 192 && p.Cb % 256 == 0) ? 256 : 192;       // (forced by the switch)
    }
    if (bn == 0) return 0;
    if (t.tn16x_phased_bn == 192 || t.tn16x_phased_bn == 256) bn = t.tn16x_phased_bn;
    return bn;
}

static bool plan_tn16x(const Tune16& t, const TN16Params& p, int nbi, int* sk_out, int* rps_out) {
    const int use_wide = t.tn16_wide;
    if (!use_wide || p.Mf <= 128 || p.M < 8 * P16_TN_BK) return false;
    // the kernel walks a power-of-two pixel grid by shifts (every BigGAN resolution is one); others take tn16_kernel
    if (p.g.k > 0 && (p.g.Wq <= 0 || p.g.Hq <= 0 || (p.g.Wq & (p.g.Wq - 1)) || (p.g.Hq & (p.g.Hq - 1)))) return false;
    // (g.k == 0: plain rows, no pixel walk)
    const int tm = (p.Mf + 255) / 256, tn = (p.Cb + 128 * nbi - 1) / (128 * nbi);
    const int wantx0 = t.tn16x_want;
    const int wantx = nbi == 2 ? wantx0 / 2 : wantx0;           // (one block per CU with the 96 KB ring)
    int sk = wantx / (tm * tn);
    const int max_sk = (p.M + 4 * P16_TN_BK - 1) / (4 * P16_TN_BK);
    if (sk > max_sk) sk = max_sk;
    if (sk < 1) sk = 1;
    if (sk > 512) sk = 512;
    int rps = (p.M + sk - 1) / sk;
    rps = (rps + P16_TN_BK - 1) / P16_TN_BK * P16_TN_BK;
    *sk_out = (p.M + rps - 1) / rps;
    *rps_out = rps;
    return true;
}


// ------------------------------------------------------------------------------------------
// the plans
// ------------------------------------------------------------------------------------------
static void plan_pow2(const Gather& g, int* pow2, int* wq_shift, int* hq_shift) {
    *pow2 = g.Wq > 0 && g.Hq > 0 && (g.Wq & (g.Wq - 1)) == 0 && (g.Hq & (g.Hq - 1)) == 0;
    *wq_shift = *pow2 ? __builtin_ctz(g.Wq) : 0;
    *hq_shift = *pow2 ? __builtin_ctz(g.Hq) : 0;
}

static size_t slab_bytes(int splitk, int64_t elems) { return splitk > 1 ? (size_t)splitk * elems * sizeof(float) : 0; }

NN16Launch plan_nn16_launch(const Tune16& t, const NN16Params& p, int mode, int zdim, int64_t out_elems, bool have_ws,
                            size_t ws_bytes) {
    const Gather& g = p.g;
    NN16Launch l{};
    l.mode = mode; l.grid_z = 1;
    // the depth-to-space store: stride-1 forward gathers whose N columns are 2 x 2 blocks of d2s_c channels
    const bool d2s_shape = p.d2s_c > 0 && p.d2s_c % 8 == 0 && p.N == 4 * p.d2s_c && p.C % 8 == 0 && mode == GATHER_CONV &&
                           zdim == 1 && g.stride == 1 && g.pstep == 1 && g.Hq == g.Ho && g.Wq == g.Wo && !p.stats_part &&
                           !p.ring && (int64_t)g.Nb * g.Ho * g.Wo * 4 < (int64_t(1) << 31);
    if (const int ntaps = nn16h_taps(t, p, mode, zdim)) {
        l.family = NN16_HALO; l.nt = ntaps; l.nf = l.tn = least_padded_tile(p.N); l.splitk = 1; l.block = 512;
        l.tiles_m = g.Nb * (g.Hq / P16_HALO_T) * (g.Wq / P16_HALO_T);
        l.tiles_n = (p.N + 32 * l.nf - 1) / (32 * l.nf);
        l.grid_x = (int64_t)l.tiles_m * l.tiles_n * (g.pstep * g.pstep);
        l.mfast = nn16_mfast(t, p, l.tiles_m, l.tiles_n);
        l.stats_rows = 2 * (int64_t)l.tiles_m * (g.pstep * g.pstep);      // one per half patch
        l.d2s_store = d2s_shape;
        if (ws_bytes == (size_t)-1)
            l.ws_bytes = slab_bytes(plan_nn16(t, p, mode, zdim, nn16_posmajor_fraction(t, p, mode), true).splitk, out_elems);
        return l;
    }
    l.family = NN16_TAP;
    const double pm = nn16_posmajor_fraction(t, p, mode);
    const NN16Plan pl = plan_nn16(t, p, mode, zdim, pm, have_ws);
    // a plan made with splitting allowed whose slabs do not fit keeps its tile and runs unsplit: no re-plan
    l.splitk = ws_bytes < slab_bytes(pl.splitk, out_elems) ? 1 : pl.splitk;
    l.ws_bytes = slab_bytes(l.splitk, out_elems);
    l.posmajor = pm < 1.0;
    // the store exists with image-major rows and no split-K; what counts is the plan the UNFUSED launch of the same shape
    // would take (with a workspace), while the fused launch itself is handed none
    l.d2s_store = d2s_shape && !l.posmajor && (have_ws ? pl : plan_nn16(t, p, mode, zdim, pm, true)).splitk == 1;
    // the pipeline form: by the grid the 256-row tile would leave; the phased form brings its own column tile
    int xtn;
    l.form = nn16_form(t, p, l.posmajor, pl.tn, (int64_t)((p.M + 255) / 256) * zdim * l.splitk,
                       zdim == 1 || g.k % g.stride == 0, false, &xtn);
    l.tn = l.form == NN16_FORM_PHASED ? xtn : pl.tn;
    const int bm = (l.form == NN16_FORM_WIDE || l.form == NN16_FORM_PHASED) ? 256 : P16_BM;
    l.tiles_n = (p.N + 32 * l.tn - 1) / (32 * l.tn);
    l.tiles_m = (p.M + bm - 1) / bm;
    plan_pow2(g, &l.pow2, &l.wq_shift, &l.hq_shift);
    l.mfast = nn16_mfast(t, p, l.tiles_m, l.tiles_n);
    l.grid_x = (int64_t)l.tiles_m * l.tiles_n;
    l.grid_z = zdim * l.splitk;
    if (mode == GATHER_TCONV && zdim > 1 && l.splitk == 1 && g.k % g.stride == 0) {
        l.zfold = zdim;                     // the phases of one M tile gather the same input rows: same XCD
        l.grid_x *= zdim;
        l.grid_z = 1;
    }
    l.block = 2 * bm;                       // 256 threads at 128 rows, 512 at 256
    return l;
}

// A mirrored-tap launch has no split (slabs live in output coordinates: it touches a few lines of them), position-major
// rows over the pixels that receive mirrored taps, and its own least-padding column tile.
NN16Launch plan_nn16_ring_launch(const Tune16& t, const NN16Params& plain, int ring_lines) {
    const Gather& g = plain.g;
    NN16Launch l{};
    l.family = NN16_MIRROR_RING; l.mode = GATHER_TCONV; l.posmajor = 1; l.splitk = 1; l.grid_z = 1; l.block = 256;
    const int npos = ring_lines * g.Wo + ring_lines * (g.Ho - ring_lines);
    l.tn = least_padded_tile(plain.N);
    l.tiles_m = (g.Nb * npos + P16_BM - 1) / P16_BM;
    l.tiles_n = (plain.N + 32 * l.tn - 1) / (32 * l.tn);
    l.mfast = nn16_mfast(t, plain, l.tiles_m, l.tiles_n);
    l.grid_x = (int64_t)l.tiles_m * l.tiles_n;
    int xtn;
    l.form = nn16_form(t, plain, true, l.tn, 0, true, true, &xtn);
    return l;
}

NN16Launch plan_nn16h_d2s_launch(const NN16Params& plain) {
    NN16Launch l{};
    l.family = NN16_HALO_D2S; l.mode = GATHER_CONV; l.nt = 2; l.nf = l.tn = 1; l.splitk = 1; l.grid_z = 1; l.block = 512;
    l.tiles_m = plain.g.Nb * (plain.g.Hs / P16_HALO_T) * (plain.g.Ws / P16_HALO_T);
    l.tiles_n = 1;
    l.grid_x = l.tiles_m;
    l.d2s_store = true;
    return l;
}

// Weight gradients.  The wide kernel (or its phased form) runs only if its plan is unsplit or its slabs fit; otherwise the
// narrow kernel with its own split, or unsplit when that does not fit either or the output is not one dense block.  The
// workspace query answers the larger of the two plans.
TN16Launch plan_tn16_launch(const Tune16& t, const TN16Params& p, int mode, bool have_ws, size_t ws_bytes) {
    const int64_t total = (int64_t)p.Mf * p.Cb;
    const bool dense = p.out_ld == p.Cb;
    TN16Launch l{};
    l.mode = mode == GATHER_CONV ? GATHER_CONV : GATHER_PLAIN;
    if (mode != GATHER_PLAIN) plan_pow2(p.g, &l.pow2, &l.wq_shift, &l.hq_shift);
    int sk, rps, skx = 1, rpsx = 0;
    plan_tn16(t, p, &sk, &rps);
    const int nbi = tn16x_nbi(t, p);
    const bool wide = plan_tn16x(t, p, nbi, &skx, &rpsx);
    const size_t query_bytes = slab_bytes(wide && skx > sk ? skx : sk, total);
    if (wide && (skx == 1 || (have_ws && ws_bytes >= slab_bytes(skx, total) && dense))) {
        l.kernel = TN16_WIDE; l.splitk = skx; l.rows_per_split = rpsx; l.block = 512;
        l.tiles_m = (p.Mf + 255) / 256;
        l.tiles_n = (p.Cb + 128 * nbi - 1) / (128 * nbi);
        l.nbi = nbi;
        l.bk = nbi == 2 ? 32 : t.tn16x_bk;
        if (const int pbn = tn16x_phased_bn(t, p, mode, nbi, l.tiles_m, skx)) {
            l.kernel = TN16_PHASED; l.bn = pbn; l.nkb = t.tn16x_phased_ring == 8 ? 8 : 6;
            l.tiles_n = (p.Cb + pbn - 1) / pbn;
        }
    } else {
        if (sk > 1 && (!have_ws || ws_bytes < slab_bytes(sk, total) || !dense)) {
            sk = 1;
            rps = (p.M + P16_TN_BK - 1) / P16_TN_BK * P16_TN_BK;
        }
        l.kernel = TN16_NARROW; l.splitk = sk; l.rows_per_split = rps; l.block = 256;
        l.tiles_m = (p.Mf + 127) / 128;
        l.tiles_n = (p.Cb + 127) / 128;
    }
    l.grid_x = (int64_t)l.tiles_m * l.tiles_n * l.splitk;
    l.ws_bytes = ws_bytes == (size_t)-1 ? query_bytes : slab_bytes(l.splitk, total);
    return l;
}

// The instantiation's name, as prof_kernel records it
void nn16_launch_name(const NN16Launch& l, char* buf, size_t n) {
    const int slots = (l.form == NN16_FORM_RING || l.form == NN16_FORM_WIDE) ? 3 : 2;
    const int wm = (l.form == NN16_FORM_WIDE || l.form == NN16_FORM_PHASED) ? 4 : 2;
    const char* pm = l.posmajor ? "true" : "false";
    if (l.family == NN16_HALO) snprintf(buf, n, "nn16h_kernel<%d, %d, %d>", l.nt, l.nf, l.mode);
    else if (l.family == NN16_HALO_D2S) snprintf(buf, n, "nn16h_kernel<%d, %d, %d, d2s>", l.nt, l.nf, l.mode);
    else if (l.family == NN16_MIRROR_RING) snprintf(buf, n, "nn16_kernel<%d, %d, true, true, %d>", l.tn, l.mode, slots);
    else if (slots == 2 && wm == 2) snprintf(buf, n, "nn16_kernel<%d, %d, %s>", l.tn, l.mode, pm);
    else snprintf(buf, n, "nn16_kernel<%d, %d, %s, false, %d, %d>", l.tn, l.mode, pm, slots, wm);
}

void tn16_launch_name(const TN16Launch& l, char* buf, size_t n) {
    if (l.kernel == TN16_PHASED) snprintf(buf, n, "tn16x_phased_kernel<%d, %d, %d>", l.mode, l.bn, l.nkb);
    else if (l.kernel == TN16_NARROW) snprintf(buf, n, "tn16_kernel<%d>", l.mode);
    else if (l.nbi == 2) snprintf(buf, n, "tn16x_kernel<%d, 32, 2>", l.mode);
    else snprintf(buf, n, "tn16x_kernel<%d, %d>", l.mode, l.bk == 64 ? 64 : 32);
}

}  // namespace bg
