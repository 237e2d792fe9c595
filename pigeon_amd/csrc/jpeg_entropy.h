// jpeg_entropy.h -- the host stage of the JPEG decoder: header parsing, the coefficient layout and the Huffman decode.
// Plain C++, no HIP: jpeg.hip includes it for the library, and a stand-alone program can include it alone (tests build one with the
// host compiler's sanitizers).  Everything here is bounded by (data, n) on the read side and by the image's coefficient region on the
// write side, whatever the bytes are.
//
// Supported: baseline / extended sequential Huffman (SOF0, SOF1), 8-bit samples, one interleaved scan, 1 component (grey) or 3
// components libjpeg reads as YCbCr, luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma.  Everything else is REFUSED with a reason
// code (PG_JPEG_R_*), which is not an error: the caller decodes such a file elsewhere.  A supported file whose scan is damaged is an
// ERROR: this stage does not emulate libjpeg's warn-and-fill behaviour.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/pigeon_hip.h"

namespace pgjpeg {

// zigzag position -> natural (row-major) position in the 8 x 8 block
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline const char* reason_text(int r) {
    switch (r) {
        case PG_JPEG_R_OK: return "supported";
        case PG_JPEG_R_NOT_JPEG: return "not a JPEG file";
        case PG_JPEG_R_PROGRESSIVE: return "progressive JPEG (SOF2)";
        case PG_JPEG_R_LOSSLESS: return "lossless JPEG";
        case PG_JPEG_R_HIERARCHICAL: return "hierarchical JPEG";
        case PG_JPEG_R_ARITHMETIC: return "arithmetic coding";
        case PG_JPEG_R_PRECISION: return "sample precision is not 8 bits";
        case PG_JPEG_R_COMPONENTS: return "component count is not 1 or 3";
        case PG_JPEG_R_COLORSPACE: return "three components that are not YCbCr";
        case PG_JPEG_R_SAMPLING: return "sampling other than 4:4:4, 4:2:2 (2x1) or 4:2:0";
        case PG_JPEG_R_MULTISCAN: return "more than one scan";
        case PG_JPEG_R_DNL: return "DNL marker";
        case PG_JPEG_R_SIZE: return "height or width is 0 or above 16384";
        case PG_JPEG_R_MALFORMED: return "malformed or truncated header";
    }
    return "unknown reason";
}

struct HuffSpec {
    bool set = false;
    uint8_t bits[17] = {0};          // bits[l] = number of codes of length l, l = 1..16
    uint8_t vals[256] = {0};
};

struct Header {
    int reason = PG_JPEG_R_OK;
    int height = 0, width = 0, ncomp = 0, hs = 0, vs = 0;
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool qt_set[4] = {false, false, false, false};
    uint16_t qt[4][64];              // natural order
    HuffSpec dc[4], ac[4];
    int restart_interval = 0;
    size_t scan_start = 0;           // offset of the first entropy-coded byte
};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Reads the markers up to and including SOS.  Returns the reason code (also in h->reason); height / width / ncomp are filled as far
// as the header got.
inline int parse_header(const uint8_t* d, size_t n, Header* h) {
    memset(h->qt, 0, sizeof(h->qt));
    auto refuse = [&](int r) { h->reason = r; return r; };
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return refuse(PG_JPEG_R_NOT_JPEG);
    size_t pos = 2;
    bool jfif = false, adobe = false, sof = false;
    int adobe_transform = -1;
    for (;;) {
        if (pos >= n || d[pos] != 0xFF) return refuse(PG_JPEG_R_MALFORMED);
        while (pos < n && d[pos] == 0xFF) ++pos;                   // fill bytes in front of a marker
        if (pos >= n) return refuse(PG_JPEG_R_MALFORMED);
        const int m = d[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return refuse(PG_JPEG_R_MALFORMED);   // no segment may stand here
        if (pos + 2 > n) return refuse(PG_JPEG_R_MALFORMED);
        const size_t len = (size_t)be16(d + pos);
        if (len < 2 || len > n - pos) return refuse(PG_JPEG_R_MALFORMED);
        const uint8_t* seg = d + pos + 2;
        size_t sl = len - 2;
        pos += len;
        switch (m) {
            case 0xE0:
                if (sl >= 14 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
                break;
            case 0xEE:
                if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) { adobe = true; adobe_transform = seg[11]; }
                break;
            case 0xDB:
                while (sl > 0) {
                    const int pq = seg[0] >> 4, tq = seg[0] & 15;
                    if (tq > 3 || pq > 1) return refuse(PG_JPEG_R_MALFORMED);
                    const size_t need = 1 + (size_t)64 * (1 + pq);
                    if (sl < need) return refuse(PG_JPEG_R_MALFORMED);
                    for (int i = 0; i < 64; ++i)
                        h->qt[tq][kNatural[i]] = (uint16_t)(pq ? be16(seg + 1 + 2 * i) : seg[1 + i]);
                    h->qt_set[tq] = true;
                    seg += need; sl -= need;
                }
                break;
            case 0xC4:
                while (sl > 0) {
                    const int tc = seg[0] >> 4, th = seg[0] & 15;
                    if (tc > 1 || th > 3 || sl < 17) return refuse(PG_JPEG_R_MALFORMED);
                    size_t total = 0;
                    for (int l = 1; l <= 16; ++l) total += seg[l];
                    if (total > 256 || sl < 17 + total) return refuse(PG_JPEG_R_MALFORMED);
                    HuffSpec& t = tc ? h->ac[th] : h->dc[th];
                    t.set = true;
                    t.bits[0] = 0;
                    memcpy(t.bits + 1, seg + 1, 16);
                    memset(t.vals, 0, sizeof(t.vals));
                    memcpy(t.vals, seg + 17, total);
                    seg += 17 + total; sl -= 17 + total;
                }
                break;
            case 0xC0: case 0xC1: {
                if (sof || sl < 6) return refuse(PG_JPEG_R_MALFORMED);
                sof = true;
                const int prec = seg[0], nc = seg[5];
                h->height = be16(seg + 1); h->width = be16(seg + 3); h->ncomp = nc;
                if (prec != 8) return refuse(PG_JPEG_R_PRECISION);
                if (sl != (size_t)6 + 3 * (size_t)nc) return refuse(PG_JPEG_R_MALFORMED);
                if (nc != 1 && nc != 3) return refuse(PG_JPEG_R_COMPONENTS);
                if (h->height < 1 || h->width < 1 || h->height > 16384 || h->width > 16384) return refuse(PG_JPEG_R_SIZE);
                for (int c = 0; c < nc; ++c) {
                    h->comp_id[c] = seg[6 + 3 * c];
                    h->comp_h[c] = seg[7 + 3 * c] >> 4; h->comp_v[c] = seg[7 + 3 * c] & 15;
                    h->comp_tq[c] = seg[8 + 3 * c];
                    if (h->comp_h[c] < 1 || h->comp_h[c] > 4 || h->comp_v[c] < 1 || h->comp_v[c] > 4 || h->comp_tq[c] > 3)
                        return refuse(PG_JPEG_R_MALFORMED);
                }
                break;
            }
            case 0xC2: return refuse(PG_JPEG_R_PROGRESSIVE);
            case 0xC3: return refuse(PG_JPEG_R_LOSSLESS);
            case 0xC5: case 0xC6: case 0xC7: case 0xDE: case 0xDF: return refuse(PG_JPEG_R_HIERARCHICAL);
            case 0xC9: case 0xCA: case 0xCB: case 0xCC: case 0xCD: case 0xCE: case 0xCF: return refuse(PG_JPEG_R_ARITHMETIC);
            case 0xC8: return refuse(PG_JPEG_R_MALFORMED);
            case 0xDC: return refuse(PG_JPEG_R_DNL);
            case 0xDD:
                if (sl != 2) return refuse(PG_JPEG_R_MALFORMED);
                h->restart_interval = be16(seg);
                break;
            case 0xDA: {
                if (!sof || sl < 1) return refuse(PG_JPEG_R_MALFORMED);
                const int ns = seg[0];
                if (ns < 1 || ns > 4 || sl != (size_t)4 + 2 * (size_t)ns) return refuse(PG_JPEG_R_MALFORMED);
                if (ns != h->ncomp) return refuse(PG_JPEG_R_MULTISCAN);
                for (int c = 0; c < ns; ++c) {
                    if (seg[1 + 2 * c] != h->comp_id[c]) return refuse(PG_JPEG_R_MALFORMED);
                    h->td[c] = seg[2 + 2 * c] >> 4; h->ta[c] = seg[2 + 2 * c] & 15;
                    if (h->td[c] > 3 || h->ta[c] > 3 || !h->dc[h->td[c]].set || !h->ac[h->ta[c]].set || !h->qt_set[h->comp_tq[c]])
                        return refuse(PG_JPEG_R_MALFORMED);
                }
                if (h->ncomp == 1) {
                    h->hs = h->vs = 1;                             // a one-component scan is not interleaved: its sampling factors mean nothing
                } else {
                    // what libjpeg takes for YCbCr: JFIF says so, else Adobe's transform flag, else the component ids
                    if (!jfif) {
                        if (adobe) { if (adobe_transform != 1) return refuse(PG_JPEG_R_COLORSPACE); }
                        else if (h->comp_id[0] == 'R' && h->comp_id[1] == 'G' && h->comp_id[2] == 'B') return refuse(PG_JPEG_R_COLORSPACE);
                    }
                    h->hs = h->comp_h[0]; h->vs = h->comp_v[0];
                    const bool luma_ok = (h->hs == 1 && h->vs == 1) || (h->hs == 2 && h->vs == 1) || (h->hs == 2 && h->vs == 2);
                    if (!luma_ok || h->comp_h[1] != 1 || h->comp_v[1] != 1 || h->comp_h[2] != 1 || h->comp_v[2] != 1)
                        return refuse(PG_JPEG_R_SAMPLING);
                }
                h->scan_start = pos;
                return refuse(PG_JPEG_R_OK);
            }
            default: break;                                        // APPn, COM and anything else with a length: skipped
        }
    }
}

// The padded block grid of every component: whole MCUs.
inline void block_grid(int height, int width, int ncomp, int hs, int vs, int32_t bw[3], int32_t bh[3]) {
    const int mx = (width + 8 * hs - 1) / (8 * hs), my = (height + 8 * vs - 1) / (8 * vs);
    bw[0] = mx * hs; bh[0] = my * vs;
    for (int c = 1; c < 3; ++c) { bw[c] = ncomp == 3 ? mx : 0; bh[c] = ncomp == 3 ? my : 0; }
}

// ---- Huffman tables as lookup tables -------------------------------------------------------------------------------------
static const int kLook = 9;
struct HuffTable {
    uint16_t look[1 << kLook];       // (length << 8) | symbol for codes of at most kLook bits, 0 = longer or no code
    int32_t maxcode[18];             // largest code of length l, -1 if none
    int32_t valoff[17];              // vals index of the first code of length l, minus that code
    uint8_t vals[256];
    int16_t fast[1 << kLook];        // AC tables: (value << 8) | (run << 4) | bits used, where code and value fit in kLook bits; else 0
};

inline bool build_table(const HuffSpec& s, HuffTable* t) {
    memset(t->look, 0, sizeof(t->look));
    memcpy(t->vals, s.vals, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;
        if (s.bits[l]) {
            if (code + s.bits[l] >= (1 << l)) return false;        // more codes than the length holds (the all-ones code is not one)
            for (int i = 0; i < s.bits[l]; ++i, ++k, ++code)
                if (l <= kLook) {
                    const int lo = code << (kLook - l);
                    for (int j = 0; j < (1 << (kLook - l)); ++j) t->look[lo + j] = (uint16_t)((l << 8) | s.vals[k]);
                }
            t->maxcode[l] = code - 1;
        } else {
            t->maxcode[l] = -1;
        }
        code <<= 1;
    }
    t->maxcode[17] = 0x7fffffff;
    // run, size and value in one lookup where the code and its value bits fit into the lookahead and the value into 8 bits
    for (int i = 0; i < (1 << kLook); ++i) {
        t->fast[i] = 0;
        const int e = t->look[i];
        if (!e) continue;
        const int len = e >> 8, run = (e >> 4) & 15, mag = e & 15;
        if (mag == 0 || len + mag > kLook) continue;
        int v = ((i << len) & ((1 << kLook) - 1)) >> (kLook - mag);
        if (v < (1 << (mag - 1))) v += 1 - (1 << mag);
        if (v >= -128 && v <= 127) t->fast[i] = (int16_t)(v * 256 + run * 16 + len + mag);
    }
    return true;
}

// ---- bit reader over the scan: stuffed FF 00 undone, stops in front of a marker and at the end of the data ----------------
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;                // the low `cnt` bits are data not yet consumed
    int cnt = 0;
    void fill() {
        while (cnt <= 32 && end - p >= 4) {                        // four bytes at once where none of them is FF
            const uint32_t v = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            if ((~v - 0x01010101u) & v & 0x80808080u) break;
            acc = (acc << 32) | v;
            cnt += 32;
            p += 4;
        }
        while (cnt <= 56) {
            if (p >= end) return;
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (p + 1 >= end) return;
                if (p[1] != 0x00) return;                          // a marker (or fill bytes in front of one): not consumed
                p += 2;
            } else {
                p += 1;
            }
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }
    // the next nb bits (nb <= 16), zero-padded where the data has run out: the caller checks the code length against cnt
    uint32_t peek(int nb) const {
        return (uint32_t)((cnt >= nb ? acc >> (cnt - nb) : acc << (nb - cnt)) & ((1u << nb) - 1));
    }
};

enum { E_NONE = 0, E_CODE = 1, E_DATA = 2, E_INDEX = 3, E_RST = 4, E_EOI = 5, E_TABLE = 6, E_HEADER = 7, E_LAYOUT = 8, E_DCSIZE = 9 };

inline const char* error_text(int e) {
    switch (e) {
        case E_CODE: return "a Huffman code that does not exist";
        case E_DATA: return "a marker or the end of the data inside an MCU";
        case E_INDEX: return "a coefficient index past 63";
        case E_RST: return "a missing or out-of-sequence RSTn marker";
        case E_EOI: return "no EOI marker behind the last MCU";
        case E_TABLE: return "an invalid Huffman table";
        case E_HEADER: return "the file is not one this decoder supports";
        case E_LAYOUT: return "the descriptor does not belong to this file or its coefficient region leaves the buffer";
        case E_DCSIZE: return "a DC size category above 15";
    }
    return "no error";
}

static inline int decode_symbol(Bits& b, const HuffTable& t, int* err) {
    if (b.cnt < 16) b.fill();
    const uint32_t e = t.look[b.peek(kLook)];
    if (e) {
        const int len = (int)(e >> 8);
        if (len > b.cnt) { *err = E_DATA; return -1; }
        b.cnt -= len;
        return (int)(e & 255);
    }
    int l = kLook + 1;
    int32_t code = (int32_t)b.peek(l);
    while (l <= 16 && code > t.maxcode[l]) { ++l; if (l <= 16) code = (int32_t)b.peek(l); }
    if (l > 16) { *err = b.cnt < 16 ? E_DATA : E_CODE; return -1; }
    if (l > b.cnt) { *err = E_DATA; return -1; }
    b.cnt -= l;
    return t.vals[(code + t.valoff[l]) & 255];
}

// s bits as a signed value of category s (1 <= s <= 15)
static inline int receive_extend(Bits& b, int s, int* err) {
    if (b.cnt < s) { b.fill(); if (b.cnt < s) { *err = E_DATA; return 0; } }
    const int v = (int)((b.acc >> (b.cnt - s)) & ((1u << s) - 1));
    b.cnt -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: 64 int16 in natural order at blk (zero on entry).  *pred is the component's DC predictor (wraps in 32 bits).
static inline int decode_block(Bits& b, const HuffTable& dc, const HuffTable& ac, uint32_t* pred, int16_t* blk) {
    int err = E_NONE;
    int s = decode_symbol(b, dc, &err);
    if (s < 0) return err;
    if (s > 15) return E_DCSIZE;
    if (s) {
        const int diff = receive_extend(b, s, &err);
        if (err) return err;
        *pred += (uint32_t)diff;
    }
    blk[0] = (int16_t)(*pred & 0xffff);
    for (int k = 1; k < 64;) {
        if (b.cnt < 16) b.fill();
        const int f = ac.fast[b.peek(kLook)];
        if (f) {
            const int used = f & 15;
            if (used > b.cnt) return E_DATA;
            k += (f >> 4) & 15;
            if (k > 63) return E_INDEX;
            b.cnt -= used;
            blk[kNatural[k++]] = (int16_t)(f >> 8);
            continue;
        }
        const int rs = decode_symbol(b, ac, &err);
        if (rs < 0) return err;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return E_INDEX;
            const int v = receive_extend(b, s, &err);
            if (err) return err;
            blk[kNatural[k]] = (int16_t)v;
            ++k;
        } else {
            if (r != 15) break;                                    // end of block
            k += 16;
            if (k > 64) return E_INDEX;
        }
    }
    return E_NONE;
}

// In front of a marker: the bits left in the accumulator are padding (fewer than 8), fill bytes may follow.  Returns the marker's
// code and steps over it, or -1.
static inline int take_marker(Bits& b) {
    if (b.cnt >= 8) return -1;                                     // whole unread bytes in front of the marker
    b.cnt = 0; b.acc = 0;
    if (b.p + 1 >= b.end || b.p[0] != 0xFF) return -1;
    while (b.p + 1 < b.end && b.p[1] == 0xFF) ++b.p;
    if (b.p + 1 >= b.end) return -1;
    const int m = b.p[1];
    b.p += 2;
    return m;
}

// Decodes one file into its coefficient region.  `it` holds the image's layout (pg_jpeg_plan); on success its quantisation tables and
// table selectors are filled in.  coef: the HOST coefficient buffer of coef_bytes bytes the offsets refer to.  Returns E_*.
inline int decode_image(const uint8_t* d, size_t n, pg_jpeg_item* it, uint8_t* coef, size_t coef_bytes) {
    Header h;
    if (parse_header(d, n, &h) != PG_JPEG_R_OK) return E_HEADER;
    int32_t bw[3], bh[3];
    block_grid(h.height, h.width, h.ncomp, h.hs, h.vs, bw, bh);
    if (it->height != h.height || it->width != h.width || it->ncomp != h.ncomp || it->hs != h.hs || it->vs != h.vs) return E_LAYOUT;
    for (int c = 0; c < h.ncomp; ++c) {
        const size_t bytes = (size_t)bw[c] * bh[c] * 128;
        if (it->bw[c] != bw[c] || it->bh[c] != bh[c] || it->coef_off[c] % 16 || it->coef_off[c] > coef_bytes ||
            bytes > coef_bytes - it->coef_off[c])
            return E_LAYOUT;
    }
    HuffTable tdc[3], tac[3];
    for (int c = 0; c < h.ncomp; ++c)
        if (!build_table(h.dc[h.td[c]], &tdc[c]) || !build_table(h.ac[h.ta[c]], &tac[c])) return E_TABLE;
    int16_t* base[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < h.ncomp; ++c) {
        base[c] = (int16_t*)(coef + it->coef_off[c]);
        memset(base[c], 0, (size_t)bw[c] * bh[c] * 128);
    }
    const int hc[3] = {h.hs, 1, 1}, vc[3] = {h.vs, 1, 1};
    const int mcux = bw[0] / h.hs, mcuy = bh[0] / h.vs;
    Bits b;
    b.p = d + h.scan_start; b.end = d + n;
    uint32_t pred[3] = {0, 0, 0};
    int64_t mcu = 0;
    int rst = 0;
    for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx, ++mcu) {
            if (h.restart_interval && mcu && mcu % h.restart_interval == 0) {
                if (take_marker(b) != 0xD0 + (rst & 7)) return E_RST;
                ++rst;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.ncomp; ++c)
                for (int v = 0; v < vc[c]; ++v)
                    for (int u = 0; u < hc[c]; ++u) {
                        const size_t blk = (size_t)(my * vc[c] + v) * bw[c] + (size_t)(mx * hc[c] + u);
                        const int e = decode_block(b, tdc[c], tac[c], &pred[c], base[c] + blk * 64);
                        if (e) return e;
                    }
        }
    if (take_marker(b) != 0xD9) return E_EOI;
    memcpy(it->qt, h.qt, sizeof(h.qt));
    for (int c = 0; c < 3; ++c) it->qsel[c] = c < h.ncomp ? h.comp_tq[c] : 0;
    return E_NONE;
}

}  // namespace pgjpeg
