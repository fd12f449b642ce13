// powerspec_fft.h - the index arithmetic of the LDS FFT of powerspec.hip: plain C++ that compiles for the host as well, so
// that the pass schedule, the padded layouts and the butterflies can be run over a thread loop on a CPU.
//
// One buffer holds POINTS = G * S complex numbers: G sequences of length S = 1 << lg, element i of sequence q at the
// logical index e = q * S + i, real and imaginary parts in two float planes (every LDS access is a 4-byte one: 32 banks,
// lane groups of 32).  The transform is a Stockham autosort (decimation in frequency, no bit reversal): radix-4 passes with
// (n, s) = (S, 1), (S / 4, 4), ... and, for odd lg, one last radix-2 pass; pass k reads buffer k & 1 and writes the other.
//
// Banks.  Butterfly j of a sequence reads the logical elements j + k * S / 4 (k = 0..3): consecutive lanes read
// consecutive words whatever the pass.  It writes q + s * (4 p + k) with j = p * s + q: runs of s consecutive words that
// lie 4 s apart - for s = 1, 4 and 16 a stride of 4, 16 or 64 words between runs, a power of two, which is the worst case
// for 32 banks.  Since reads are unit-stride under any monotone padding, every pass pads the buffer it WRITES for its own
// stride and the next pass reads through the same map:
//     mode 1 (s = 1)    e + (e >> 5)          32 runs of 1, 4 apart: +1 every 32 words, all 32 banks once
//     mode 2 (s = 4)    e + 4 * (e >> 5)      8 runs of 4, 16 apart: +4 every 32 words, all 32 banks once
//     mode 3 (s = 16)   e + 16 * (e >> 6)     2 runs of 16, 64 apart: +16 every 64 words, all 32 banks once
//     mode 0 (s >= 32)  e                     a lane group is one run
//     mode 4            e + sk * (e >> lg)    the column kernel's staging and read-out: lanes run across sequences, which
//                                             are S words apart; sk = max(1, 32 / G) words of skew per sequence
// A buffer plane therefore holds POINTS + POINTS / 4 floats.  (Unit-stride reads through modes 1-3 cross at most one gap
// per lane group: one 2-way conflict at worst.  Sides 16 and 32 keep lanes of several sequences in one group and are not
// conflict-free in every pass; they are also the sides whose whole transform is a few hundred butterflies.)
#pragma once

#if defined(__HIPCC__)
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif

PS_HD int ps_phys(int e, int mode, int lg, int sk) {
    switch (mode) {
        case 1: return e + (e >> 5);
        case 2: return e + ((e >> 5) << 2);
        case 3: return e + ((e >> 6) << 4);
        case 4: return e + (e >> lg) * sk;
        default: return e;
    }
}

struct PsPass {
    int radix, ln, ls;      // n = 1 << ln points per sub-transform, stride s = 1 << ls; n * s = S
    int rmode, wmode;       // layouts of the buffer read and of the buffer written
};

// Pass after pass of a length-(1 << lg) transform whose input lies in layout mode_in: start from ps_first_pass and call
// ps_next_pass until it returns false.  The last pass writes in layout final_mode when its runs are at least a lane
// group long (s >= 32) and in its own padded layout otherwise.
PS_HD void ps_set_pass(PsPass* p, int ln, int ls, int rmode, int final_mode) {
    p->radix = ln >= 2 ? 4 : 2;
    p->ln = ln;
    p->ls = ls;
    p->rmode = rmode;
    const int s = 1 << ls;
    p->wmode = (ln <= 2 && s >= 32) ? final_mode : (p->radix == 4 ? (s == 1 ? 1 : s == 4 ? 2 : s == 16 ? 3 : 0) : 0);
}

PS_HD PsPass ps_first_pass(int lg, int mode_in, int final_mode) {
    PsPass p;
    ps_set_pass(&p, lg, 0, mode_in, final_mode);
    return p;
}

PS_HD bool ps_next_pass(PsPass* p, int final_mode) {
    const int step = p->radix == 4 ? 2 : 1;
    if (p->ln - step < 1) return false;
    ps_set_pass(p, p->ln - step, p->ls + step, p->wmode, final_mode);
    return true;
}

// Radix-4 butterfly b of POINTS / 4: sequence b >> (lg - 2), butterfly j = b & (S / 4 - 1) = p * s + q.  twr / twi hold
// exp(-2 pi i k / S) for k < S (k = p * s, 2 p s, 3 p s < 3 S / 4 are read).
PS_HD void ps_radix4(const float* xr, const float* xi, float* yr, float* yi, const float* twr, const float* twi, int b, int lg,
                     const PsPass ps, int sk) {
    const int quarter = 1 << (lg - 2);
    const int base = (b >> (lg - 2)) << lg, j = b & (quarter - 1);
    const int p = j >> ps.ls, q = j & ((1 << ps.ls) - 1);
    const int i0 = ps_phys(base + j, ps.rmode, lg, sk), i1 = ps_phys(base + j + quarter, ps.rmode, lg, sk);
    const int i2 = ps_phys(base + j + 2 * quarter, ps.rmode, lg, sk), i3 = ps_phys(base + j + 3 * quarter, ps.rmode, lg, sk);
    const float ar = xr[i0], ai = xi[i0], br = xr[i1], bi = xi[i1], cr = xr[i2], ci = xi[i2], dr = xr[i3], di = xi[i3];
    const float apcr = ar + cr, apci = ai + ci, amcr = ar - cr, amci = ai - ci;
    const float bpdr = br + dr, bpdi = bi + di;
    const float jr = -(bi - di), ji = br - dr;                       // i * (b - d)
    const float y0r = apcr + bpdr, y0i = apci + bpdi;
    const float t1r = amcr - jr, t1i = amci - ji;                    // a - i b - c + i d
    const float t2r = apcr - bpdr, t2i = apci - bpdi;
    const float t3r = amcr + jr, t3i = amci + ji;
    const int k1 = p << ps.ls;
    const float w1r = twr[k1], w1i = twi[k1], w2r = twr[2 * k1], w2i = twi[2 * k1], w3r = twr[3 * k1], w3i = twi[3 * k1];
    const int o = base + q + ((4 * p) << ps.ls), s = 1 << ps.ls;
    const int o0 = ps_phys(o, ps.wmode, lg, sk), o1 = ps_phys(o + s, ps.wmode, lg, sk);
    const int o2 = ps_phys(o + 2 * s, ps.wmode, lg, sk), o3 = ps_phys(o + 3 * s, ps.wmode, lg, sk);
    yr[o0] = y0r;
    yi[o0] = y0i;
    yr[o1] = t1r * w1r - t1i * w1i;
    yi[o1] = t1r * w1i + t1i * w1r;
    yr[o2] = t2r * w2r - t2i * w2i;
    yi[o2] = t2r * w2i + t2i * w2r;
    yr[o3] = t3r * w3r - t3i * w3i;
    yi[o3] = t3r * w3i + t3i * w3r;
}

// Radix-2 butterfly b of POINTS / 2 of the last pass of an odd lg (n = 2, s = S / 2): no twiddle.
PS_HD void ps_radix2(const float* xr, const float* xi, float* yr, float* yi, int b, int lg, const PsPass ps, int sk) {
    const int half = 1 << (lg - 1);
    const int base = (b >> (lg - 1)) << lg, q = b & (half - 1);
    const int i0 = ps_phys(base + q, ps.rmode, lg, sk), i1 = ps_phys(base + q + half, ps.rmode, lg, sk);
    const int o0 = ps_phys(base + q, ps.wmode, lg, sk), o1 = ps_phys(base + q + half, ps.wmode, lg, sk);
    const float ar = xr[i0], ai = xi[i0], br = xr[i1], bi = xi[i1];
    yr[o0] = ar + br;
    yi[o0] = ai + bi;
    yr[o1] = ar - br;
    yi[o1] = ai - bi;
}
