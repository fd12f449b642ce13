// igemm16_plan.h - launch plans of the bf16-resident implicit-GEMM kernels (igemm16.hip).
//
// Host only: no HIP runtime call, no kernel symbol, nothing from igemm16.hip (the pair links into a host program alone).
// A plan function takes the parameter block a pass has filled from its descriptor and decides everything about the launch - kernel family, pipeline form, tiles, split-K, row order, grid,
// workspace - ONCE; the workspace / statistics / depth-to-space queries, bg_conv_plan_describe and the launchers of
// igemm16.hip all read the same struct, so they agree by construction.  The measured rules (per-layer tables) live
// with their predicates in igemm16_plan.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "igemm16.h"

namespace bg {

// Tile constants of the kernels that the plans count with (igemm16.hip asserts them against its own).
constexpr int P16_BM = 128;       // rows of the tap kernel's block tile (256 in the wide and phased forms)
constexpr int P16_HALO_T = 16;    // patch edge of the halo-tile kernel
constexpr int P16_TN_BK = 64;     // pixels per K step of the weight-gradient kernels

// The switches of this path, one table.  once: read when the first plan is made; call: read by every tune16() (the form
// tests flip them between calls).  An entry point of igemm.hip reads them ONCE, when it makes its ConvPlan, and hands the
// same Tune16 to the route predicate and to every plan of the call.
struct Tune16 {
    int nn16_slots;          // BG_NN16_SLOTS (once; 512): co-resident blocks per round in plan_nn16's cost model
    int halo_cmax;           // BG_NN16_HALO_CMAX (once; 4096): most channels per tap the halo-tile form takes
    int tn16_want;           // BG_TN16_WANT (once; 1024): blocks tn16_kernel's split-K aims at
    int tn16_wide;           // BG_TN16_WIDE (once; 1): 0 keeps every weight gradient on tn16_kernel
    int tn16x_want;          // BG_TN16X_WANT (once; 512): blocks tn16x_kernel's split-K aims at (halved under NBI = 2)
    int tn16x_bk;            // BG_TN16X_BK (once; 32): 64 = tn16x_kernel's 64-pixel K step
    int posmajor;            // BG_NN16_POSMAJOR (call; 1): 0 switches position-major rows off
    int pipe_set, pipe;      // BG_NN16_PIPE (call; unset: the rule): 1 ring, 2 wide, 3 phased form, any other value two stages
    int nn16x_bn;            // BG_NN16X_BN (call; 0): 128 | 192 | 256 overrides the phased form's column tile
    int halo;                // BG_NN16_HALO (call; 1): 0 switches the halo-tile form off
    int halo_k3s2;           // BG_NN16_HALO_K3S2 (call; 0): 1 sends k3 s2 transposed gathers to the halo-tile form
    int thin_d2s;            // BG_THIN_D2S (call; 1): 0 switches the thin depth-to-space form off
    int mfast;               // BG_NN16_MFAST (call; 0): 1 M-tiles fastest, 2 ("auto") the fabric-bytes rule
    int tn16x_nbi;           // BG_TN16X_NBI (call; 1): 2 = 256-wide output tiles where they divide the channels
    int tn16x_phased;        // BG_TN16X_PHASED (call; -1 = unset, the rule): 0 never, 1 every launch the wide form accepts
    int tn16x_phased_bn;     // BG_TN16X_PHASED_BN (call; 0): 192 | 256 sets the phased form's column tile
    int tn16x_phased_ring;   // BG_TN16X_PHASED_RING (call; 6): K blocks of the phased form's ring, 8 = 128 KB (A/B)
};
Tune16 tune16();

enum { NN16_FORM_TWO = 0, NN16_FORM_RING = 1, NN16_FORM_WIDE = 2, NN16_FORM_PHASED = 3 };
enum { NN16_TAP = 0, NN16_HALO = 1, NN16_HALO_D2S = 2, NN16_MIRROR_RING = 3 };

struct NN16Launch {
    int family;              // NN16_TAP (nn16_kernel), NN16_HALO / NN16_HALO_D2S (nn16h_kernel), NN16_MIRROR_RING
    int mode;                // GATHER_* of the instantiation
    int form;                // NN16_FORM_* (tap and mirrored-tap launches; halo launches: NN16_FORM_TWO)
    int tn;                  // column tile / 32: 1 .. 4, the phased form 4 | 6 | 8; halo-tile launches: = nf
    int nt, nf;              // halo-tile launches: taps per axis of the window (2 | 3), column tile / 32; else 0
    int splitk, posmajor, mfast, zfold, pow2, wq_shift, hq_shift, tiles_m, tiles_n;
    int64_t grid_x;          // blocks along x (the launcher rejects >= 2^31)
    int grid_z, block;       // grid z, threads per block (dynamic LDS bytes: nn16_launch_lds, with the kernels)
    size_t ws_bytes;         // split-K slabs of this launch; of a plan made for the workspace query (ws_bytes = -1) what
                             // the query answers - for a halo-tile launch, which never splits, still the tap kernel's
                             // slabs: callers size their workspace by the query, a halo launch uses none of it
    int64_t stats_rows;      // rows of NN16Params::stats_part the launch writes (halo-tile launches), else 0
    bool d2s_store;          // the launch stores depth-to-space: the thin form; p.d2s_c set and a form with that epilogue
};

enum { TN16_NARROW = 0, TN16_WIDE = 1, TN16_PHASED = 2 };

struct TN16Launch {
    int kernel;              // TN16_NARROW tn16_kernel, TN16_WIDE tn16x_kernel<mode, bk, nbi>, TN16_PHASED tn16x_phased_kernel
    int mode;                // GATHER_CONV | GATHER_PLAIN
    int bk, nbi;             // wide: pixels per K step (32 | 64), 128-column images per tile (1 | 2)
    int bn, nkb;             // phased: column tile (192 | 256), K blocks of the ring (6 | 8)
    int splitk, rows_per_split, tiles_m, tiles_n, pow2, wq_shift, hq_shift;
    int64_t grid_x;
    int block;
    size_t ws_bytes;         // slabs of this launch; of a query plan the larger of the narrow and the wide plan's
};

// The plain launch of a forward pass / input gradient.  have_ws: the caller hands a workspace (a plan made without one
// may choose another tile than a plan whose slabs then do not fit ws_bytes: that one keeps its tile and runs unsplit).
NN16Launch plan_nn16_launch(const Tune16& t, const NN16Params& p, int mode, int zdim, int64_t out_elems, bool have_ws,
                            size_t ws_bytes);
// The mirrored-tap launch (NN16Params::ring) that follows the plain launch of block `plain`; ring_lines 1 or 2.
NN16Launch plan_nn16_ring_launch(const Tune16& t, const NN16Params& plain, int ring_lines);
// The thin depth-to-space form of an 8-channel stride-2 input gradient, for the geometries nn16h_d2s_ok accepts: the
// route predicate of the input gradient (igemm.hip plan_conv_dgrad), the one place that asks it.
bool nn16h_d2s_ok(const Tune16& t, const NN16Params& p);
NN16Launch plan_nn16h_d2s_launch(const NN16Params& plain);
TN16Launch plan_tn16_launch(const Tune16& t, const TN16Params& p, int mode, bool have_ws, size_t ws_bytes);

// The instantiation's name as bg_prof_dump and bg_conv_plan_describe print it.
void nn16_launch_name(const NN16Launch& l, char* buf, size_t n);
void tn16_launch_name(const TN16Launch& l, char* buf, size_t n);

}  // namespace bg
