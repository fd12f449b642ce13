// jpeg_entropy.hip - host helper of the input pipeline (data.py): the serial part of a JPEG decode, i.e. the marker
// walk and the Huffman decode of an 8-bit sequential file (ITU-T T.81; SOF0 / SOF1, 1 or 3 components, one interleaved
// scan, restart intervals).  Pure C++ on the CPU, no GPU involved; what follows the coefficients (dequantisation, IDCT,
// upsampling, colour) is csrc/jpeg.hip on the device or data.decode_jpeg in numpy.
//
//   bg_jpeg_info           headers -> BgJpegInfo (size, components, sampling, block grids, quantisation tables)
//   bg_jpeg_coefficients   the scan -> int16 [blocks][64], de-zigzagged, not dequantised; component by component,
//                          block-row major
//
// The same decisions, in the same order, as data._jpeg_parse / data._jpeg_coefficients_py, which stay the specification:
// BG_ERR_ARG for anything malformed, BG_ERR_UNSUPPORTED for what the decoder does not take.  The bytes are untrusted:
// every read is checked against n, every write against the caller's count.
#include <stdarg.h>
#include <stdint.h>
#include <string.h>

#include "../../include/biggan_hip.h"

namespace bg {
void set_error(const char* fmt, ...);

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool defined;
    int32_t mincode[17], maxcode[17], first[17];    // per code length 1..16; maxcode = -1: no code of that length
    uint8_t sym[256];
};

struct Frame {
    int w, h, ncomp, hs, vs, restart;
    int ids[3], tq[3];
    int mx, my, bw[3], bh[3];
    int64_t blocks;
    size_t scan;                                    // first byte of the entropy-coded data
    uint16_t q[4][64];
    bool q_defined[4];
    Huff huff[2][4];
    int dc[3], ac[3];
};

#define JPEG_FAIL(code, ...)        \
    do {                            \
        bg::set_error(__VA_ARGS__); \
        return code;                \
    } while (0)

int parse(const uint8_t* d, size_t n, Frame& f) {
    memset(&f, 0, sizeof(f));
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) JPEG_FAIL(BG_ERR_ARG, "not a JPEG file");
    bool have_frame = false;
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n) JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated before the scan");
        if (d[pos] != 0xFF) JPEG_FAIL(BG_ERR_ARG, "JPEG: marker expected at byte %zu", pos);
        const int m = d[pos + 1];
        if (m == 0xFF) {
            ++pos;
            continue;
        }
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9 || m == 0x00) JPEG_FAIL(BG_ERR_ARG, "JPEG: marker %02X before the scan", m);
        if (pos + 2 > n) JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated segment");
        const size_t ln = ((size_t)d[pos] << 8) | d[pos + 1];
        if (ln < 2 || ln > n - pos) JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated segment");
        size_t seg = pos + 2;
        const size_t end = pos + ln;                // <= n: everything below reads d[i] with i < end only
        if (m == 0xDB) {
            while (seg < end) {
                const int pq = d[seg] >> 4, tq = d[seg] & 15;
                if (pq > 1 || tq > 3 || seg + 1 + 64 * (size_t)(pq + 1) > end)
                    JPEG_FAIL(BG_ERR_ARG, "JPEG: bad quantisation table");
                ++seg;
                for (int k = 0; k < 64; ++k) {
                    f.q[tq][kZigzag[k]] = pq ? (uint16_t)((d[seg] << 8) | d[seg + 1]) : d[seg];
                    seg += 1 + pq;
                }
                f.q_defined[tq] = true;
            }
        } else if (m == 0xC4) {
            while (seg < end) {
                if (seg + 17 > end) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad Huffman table");
                const int tc = d[seg] >> 4, th = d[seg] & 15;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += d[seg + 1 + i];
                if (tc > 1 || th > 3 || total > 256 || seg + 17 + (size_t)total > end)
                    JPEG_FAIL(BG_ERR_ARG, "JPEG: bad Huffman table");
                Huff& t = f.huff[tc][th];
                int32_t code = 0;
                int k = 0;
                for (int len = 1; len <= 16; ++len) {
                    const int cnt = d[seg + len];
                    t.first[len] = k;
                    t.mincode[len] = code;
                    if (cnt && code + cnt > (1 << len)) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad Huffman table");
                    for (int i = 0; i < cnt; ++i) t.sym[k + i] = d[seg + 17 + k + i];
                    k += cnt;
                    code += cnt;
                    t.maxcode[len] = cnt ? code - 1 : -1;
                    code <<= 1;
                }
                t.defined = true;
                seg += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (ln != 4) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad restart interval");
            f.restart = (d[seg] << 8) | d[seg + 1];
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_frame || ln < 8) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad frame header");
            const int prec = d[seg], h = (d[seg + 1] << 8) | d[seg + 2], w = (d[seg + 3] << 8) | d[seg + 4], nc = d[seg + 5];
            if (prec != 8) JPEG_FAIL(BG_ERR_UNSUPPORTED, "JPEG: %d-bit samples (8 only)", prec);
            if (ln != 8 + 3 * (size_t)nc || h < 1 || w < 1) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad frame header");
            if (nc != 1 && nc != 3) JPEG_FAIL(BG_ERR_UNSUPPORTED, "JPEG: %d components (1 or 3)", nc);
            int ch[3], cv[3];
            for (int i = 0; i < nc; ++i) {
                f.ids[i] = d[seg + 6 + 3 * i];
                ch[i] = d[seg + 7 + 3 * i] >> 4;
                cv[i] = d[seg + 7 + 3 * i] & 15;
                f.tq[i] = d[seg + 8 + 3 * i];
                if (f.tq[i] > 3 || ch[i] < 1 || cv[i] < 1) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad frame header");
            }
            if (nc == 1) {
                f.hs = f.vs = 1;                    // one component: the MCU is one block whatever the header says
            } else {
                f.hs = ch[0];
                f.vs = cv[0];
                const bool luma = (f.hs == 1 && f.vs == 1) || (f.hs == 2 && f.vs == 1) || (f.hs == 2 && f.vs == 2);
                if (!luma || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1)
                    JPEG_FAIL(BG_ERR_UNSUPPORTED, "JPEG: sampling %dx%d, %dx%d, %dx%d (luma 1x1, 2x1 or 2x2 with chroma "
                              "1x1)", ch[0], cv[0], ch[1], cv[1], ch[2], cv[2]);
            }
            f.w = w;
            f.h = h;
            f.ncomp = nc;
            have_frame = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC8) {
            JPEG_FAIL(BG_ERR_UNSUPPORTED, "JPEG: %s (Huffman sequential files only)",
                      m == 0xC2 ? "progressive" : m == 0xCC ? "arithmetic coding" : "frame type not supported");
        } else if (m == 0xDA) {
            if (!have_frame) JPEG_FAIL(BG_ERR_ARG, "JPEG: scan before the frame header");
            const int ns = ln >= 3 ? d[seg] : 0;
            if (ns < 1 || ns > 4 || ln != 6 + 2 * (size_t)ns) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad scan header");
            bool all = ns == f.ncomp;
            for (int i = 0; all && i < ns; ++i) all = d[seg + 1 + 2 * i] == f.ids[i];
            if (!all) JPEG_FAIL(BG_ERR_UNSUPPORTED, "JPEG: a scan that does not interleave all components in frame order");
            if (d[seg + 1 + 2 * ns] != 0 || d[seg + 2 + 2 * ns] != 63 || d[seg + 3 + 2 * ns] != 0)
                JPEG_FAIL(BG_ERR_ARG, "JPEG: bad scan header");
            for (int i = 0; i < ns; ++i) {
                const int td = d[seg + 2 + 2 * i] >> 4, ta = d[seg + 2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !f.huff[0][td].defined || !f.huff[1][ta].defined || !f.q_defined[f.tq[i]])
                    JPEG_FAIL(BG_ERR_ARG, "JPEG: the scan names a table that was not defined");
                f.dc[i] = td;
                f.ac[i] = ta;
            }
            f.mx = (f.w + 8 * f.hs - 1) / (8 * f.hs);
            f.my = (f.h + 8 * f.vs - 1) / (8 * f.vs);
            f.blocks = 0;
            for (int c = 0; c < f.ncomp; ++c) {
                f.bw[c] = c == 0 ? f.mx * f.hs : f.mx;
                f.bh[c] = c == 0 ? f.my * f.vs : f.my;
                f.blocks += (int64_t)f.bw[c] * f.bh[c];
            }
            if ((uint64_t)f.blocks > 4 * (uint64_t)(n - end))       // a block takes two bits at the least
                JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated scan");
            f.scan = end;
            return BG_OK;
        }
        pos = end;
    }
}

struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint32_t acc;
    int nbits;
    bool fail;

    int bit() {
        if (nbits == 0) {
            if (pos >= n) {
                fail = true;
                return 0;
            }
            acc = d[pos++];
            if (acc == 0xFF) {
                if (pos >= n || d[pos] != 0) {
                    fail = true;
                    return 0;
                }
                ++pos;
            }
            nbits = 8;
        }
        --nbits;
        return (int)((acc >> nbits) & 1u);
    }
    // the decoded symbol, or -1 (a code that the table does not hold, or the data ran out)
    int symbol(const Huff& t) {
        int32_t code = 0;
        for (int len = 1; len <= 16; ++len) {
            code = (code << 1) | bit();
            if (fail) return -1;
            if (t.maxcode[len] >= 0 && code >= t.mincode[len] && code <= t.maxcode[len])
                return t.sym[t.first[len] + (code - t.mincode[len])];
        }
        return -1;
    }
    int receive(int s) {                            // 1 <= s <= 11
        int v = 0;
        for (int i = 0; i < s; ++i) v = (v << 1) | bit();
        return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
    }
};

int decode_scan(const uint8_t* d, size_t n, const Frame& f, int16_t* coef) {
    Bits b = {d, n, f.scan, 0u, 0, false};
    int64_t base[3] = {0, 0, 0};
    for (int c = 1; c < f.ncomp; ++c) base[c] = base[c - 1] + (int64_t)f.bw[c - 1] * f.bh[c - 1];
    int pred[3] = {0, 0, 0};
    int rst = 0;
    const int64_t mcus = (int64_t)f.mx * f.my;
    for (int64_t mcu = 0; mcu < mcus; ++mcu) {
        if (f.restart && mcu && mcu % f.restart == 0) {
            b.nbits = 0;                            // the marker is byte aligned
            if (b.pos + 2 > n || d[b.pos] != 0xFF || d[b.pos + 1] != 0xD0 + rst)
                JPEG_FAIL(BG_ERR_ARG, "JPEG: restart marker %d expected", rst);
            b.pos += 2;
            rst = (rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int64_t mr = mcu / f.mx, mc = mcu % f.mx;
        for (int c = 0; c < f.ncomp; ++c) {
            const int ch = c == 0 ? f.hs : 1, cv = c == 0 ? f.vs : 1;
            const Huff& dc = f.huff[0][f.dc[c]];
            const Huff& ac = f.huff[1][f.ac[c]];
            for (int by = 0; by < cv; ++by) {
                for (int bx = 0; bx < ch; ++bx) {
                    // (mr * cv + by) < bh[c] and (mc * ch + bx) < bw[c]: the block lies inside coef[0 : 64 * blocks]
                    int16_t* blk = coef + 64 * (base[c] + (mr * cv + by) * f.bw[c] + mc * ch + bx);
                    int s = b.symbol(dc);
                    if (s < 0) JPEG_FAIL(BG_ERR_ARG, b.fail ? "JPEG: truncated scan" : "JPEG: bad Huffman code");
                    if (s > 11) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad DC category");
                    if (s) pred[c] += b.receive(s);
                    if (b.fail) JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated scan");
                    if (pred[c] < -32768 || pred[c] > 32767) JPEG_FAIL(BG_ERR_ARG, "JPEG: DC value out of range");
                    blk[0] = (int16_t)pred[c];
                    int k = 1;
                    while (k < 64) {
                        const int rs = b.symbol(ac);
                        if (rs < 0) JPEG_FAIL(BG_ERR_ARG, b.fail ? "JPEG: truncated scan" : "JPEG: bad Huffman code");
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63 || s > 10) JPEG_FAIL(BG_ERR_ARG, "JPEG: bad AC coefficient");
                        blk[kZigzag[k]] = (int16_t)b.receive(s);
                        if (b.fail) JPEG_FAIL(BG_ERR_ARG, "JPEG: truncated scan");
                        ++k;
                    }
                }
            }
        }
    }
    size_t pos = b.pos;
    while (pos + 1 < n && d[pos] == 0xFF && d[pos + 1] == 0xFF) ++pos;
    if (pos + 2 > n || d[pos] != 0xFF || d[pos + 1] != 0xD9)
        JPEG_FAIL(BG_ERR_ARG, "JPEG: no end-of-image marker after the scan");
    return BG_OK;
}

}  // namespace
}  // namespace bg

extern "C" {

int bg_jpeg_info(const unsigned char* data, size_t n, BgJpegInfo* info) {
    if (!data || !info) JPEG_FAIL(BG_ERR_ARG, "bg_jpeg_info: NULL argument");
    bg::Frame f;
    const int rc = bg::parse(data, n, f);
    if (rc != BG_OK) return rc;
    memset(info, 0, sizeof(*info));
    info->width = f.w;
    info->height = f.h;
    info->ncomp = f.ncomp;
    info->hs = f.hs;
    info->vs = f.vs;
    info->restart = f.restart;
    info->blocks = f.blocks;
    for (int c = 0; c < f.ncomp; ++c) {
        info->bw[c] = f.bw[c];
        info->bh[c] = f.bh[c];
        memcpy(info->q[c], f.q[f.tq[c]], sizeof(info->q[c]));
    }
    return BG_OK;
}

int bg_jpeg_coefficients(const unsigned char* data, size_t n, int16_t* coef, size_t coef_count) {
    if (!data || !coef) JPEG_FAIL(BG_ERR_ARG, "bg_jpeg_coefficients: NULL argument");
    bg::Frame f;
    const int rc = bg::parse(data, n, f);
    if (rc != BG_OK) return rc;
    if ((uint64_t)coef_count != 64 * (uint64_t)f.blocks)
        JPEG_FAIL(BG_ERR_ARG, "bg_jpeg_coefficients: coef_count %zu, the file has %lld blocks of 64", coef_count,
                  (long long)f.blocks);
    memset(coef, 0, sizeof(int16_t) * coef_count);
    return bg::decode_scan(data, n, f, coef);
}

}  // extern "C"
