// Baseline JPEG decode on gfx950: Image.open + np.asarray of SurgDataset.__getitem__ (dino-main/main_dino.py:295-316)
// for the feature extraction of extract_representations.py:158-162, bit-identical to libjpeg-turbo at Pillow's
// defaults.  tests/jpeg_ref.py restates every rule in numpy.
//
// Phases (one stable kernel name each):
//   jpeg_layout      per-image regions of the workspace (prefix sums of the images' own sizes), header checks
//   jpeg_destuff     one workgroup per image: drop stuffed 0x00 / fill 0xFF, cut at RSTn, stop at any other marker.
//                    Restart segment s is written at a SUB_BYTES-aligned offset, so a segment start is always the
//                    start of a subsequence (a hard sync point) and every segment is followed by >= SUB_BYTES zeros.
//   jpeg_sync_spec   one thread per SUB_BYTES subsequence: speculative Huffman decode from a guessed state
//   jpeg_sync_pass   (bounded number of launches) re-decode the subsequences whose entry state changed, until no
//                    entry changes (self-synchronising decode, Weissenberger & Schmidt, ICPP 2018 / HiPC 2021)
//   jpeg_block_scan  per image: segmented exclusive scan of the blocks started per subsequence
//   jpeg_huff_write  decode again from the converged states and write int16 coefficients in natural order
//   jpeg_dc_scan     per (image, component): DC prediction = prefix sum of the differences, reset at every restart
//   jpeg_idct        jidctint.c jpeg_idct_islow, one thread per block, into padded uint8 planes
//   jpeg_color       fancy upsampling (jdsample.c) + ycc_rgb_convert (jdcolor.c) -> interleaved RGB
// Decoder state at a codeword start: (bit position, block slot within the MCU, zig-zag index k).
//
// Every image carries its own geometry in its ImgRec.  sais_jpeg_decode (one geometry per batch, output [n,H,W,3]) and
// sais_jpeg_decode_mixed (any geometry per image, output at the caller's offsets) run the same kernels; launch grids are
// sized by the largest image and threads past an image's own count return.
#include "common.hpp"
#include "../../include/sais_hip.h"
#include <string.h>

namespace {

constexpr int SUB_BYTES = 128;            // subsequence = 1024 bits
constexpr int MAX_PASSES = 32;            // jpeg_sync_spec + 31 jpeg_sync_pass launches
constexpr int WARMUP = 6;                 // jpeg_sync_spec guesses a subsequence's entry by decoding the 6 before it
constexpr int NT = 256;

struct ImgRec {
    long long ds_off;                     // destuffed region of the image (bytes, SUB_BYTES-aligned)
    long long coef_off;                   // first block of the image in the coefficient region
    long long plane_off;                  // its planes (bytes): Y first, then Cb, Cr of cplane bytes each
    long long yplane, cplane;
    long long out_off;                    // its uint8 [H,W,3] output (bytes into out)
    int ds_cap, sub_base, nsub, seg_base, nseg;
    int H, W;
    int mcux, mcuy, bpm, ny, hs, vs, ri, blocks;
    int ystride, cstride;                 // padded plane widths
};

struct Layout {
    size_t rec, segk, sego, sege, ds, en, ex, base, flags, coef, planes, total;
    long long ds_cap, nsub;
    long long coef_cap;                   // blocks of the whole batch
    long long plane_cap;                  // plane bytes of the whole batch
};

static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// What a header says about its image: sampling, MCU grid, blocks, plane sizes.  False for a header no kernel may follow.
__host__ __device__ inline bool image_geometry(const SaisJpegHeader& h, ImgRec& r) {
    const int hs = h.hsamp, vs = h.vsamp;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    if (h.height < 1 || h.height > 65535 || h.width < 1 || h.width > 65535 || h.restart_interval < 0) return false;
    r.hs = hs; r.vs = vs; r.H = h.height; r.W = h.width;
    r.mcux = (h.width + 8 * hs - 1) / (8 * hs);
    r.mcuy = (h.height + 8 * vs - 1) / (8 * vs);
    r.ny = hs * vs;
    r.bpm = r.ny + 2;
    r.ri = h.restart_interval;
    r.blocks = r.mcux * r.mcuy * r.bpm;
    r.ystride = r.mcux * hs * 8;
    r.cstride = r.mcux * 8;
    r.yplane = (long long)r.ystride * r.mcuy * vs * 8;
    r.cplane = (long long)r.cstride * r.mcuy * 8;
    const int mcus = r.mcux * r.mcuy;
    r.nseg = r.ri ? (mcus + r.ri - 1) / r.ri : 1;
    return true;
}

__host__ __device__ inline long long plane_bytes_of(const ImgRec& r) { return (r.yplane + 2 * r.cplane + 255) & ~255LL; }
__host__ __device__ inline long long quads_of(const ImgRec& r) { return (long long)r.H * ((r.W + 3) / 4); }

// regions for `coef_cap` blocks and `plane_cap` plane bytes in all
static Layout layout_sums(int n, long long scan_bytes, int segments, long long coef_cap, long long plane_cap) {
    Layout L{};
    L.coef_cap = coef_cap;
    L.plane_cap = plane_cap;
    L.ds_cap = scan_bytes + 2LL * SUB_BYTES * segments + 3LL * SUB_BYTES * n;
    L.ds_cap = (L.ds_cap + SUB_BYTES - 1) / SUB_BYTES * SUB_BYTES;
    L.nsub = L.ds_cap / SUB_BYTES;
    size_t o = 0;
    L.rec = o;    o = al(o + sizeof(ImgRec) * (size_t)n);
    L.segk = o;   o = al(o + 4 * (size_t)segments);
    L.sego = o;   o = al(o + 4 * (size_t)segments);
    L.sege = o;   o = al(o + 4 * (size_t)segments);
    L.ds = o;     o = al(o + (size_t)L.ds_cap);
    L.en = o;     o = al(o + 8 * (size_t)L.nsub);
    L.ex = o;     o = al(o + 8 * (size_t)L.nsub);
    L.base = o;   o = al(o + 4 * (size_t)L.nsub);
    L.flags = o;  o = al(o + 4 * (size_t)MAX_PASSES * n);
    L.coef = o;   o = al(o + 128 * (size_t)coef_cap);
    L.planes = o; o = al(o + (size_t)plane_cap);
    L.total = o;
    return L;
}

// one geometry per batch: n slots of the largest block count and plane size any sampling gives that geometry
static Layout layout_of(int n, int H, int W, long long scan_bytes, int segments, int* max_blocks) {
    long long bx8 = (W + 7) / 8, by8 = (H + 7) / 8, bx16 = (W + 15) / 16, by16 = (H + 15) / 16;
    long long cb = 3 * bx8 * by8;
    if (4 * bx16 * by8 > cb) cb = 4 * bx16 * by8;
    if (6 * bx16 * by16 > cb) cb = 6 * bx16 * by16;
    const long long yplane = bx16 * 16 * by16 * 16, cplane = bx8 * 8 * by8 * 8;
    const long long plane_bytes = (yplane + 2 * cplane + 255) & ~255LL;
    if (max_blocks) *max_blocks = (int)cb;
    return layout_sums(n, scan_bytes, segments, cb * n, plane_bytes * n);
}

// any geometry per image: the sums of the images' own sizes.  A header image_geometry refuses adds nothing (jpeg_layout
// flags it and gives it no region).
struct MixedSums { long long scan, blocks, planes, max_quads, segments; int max_blocks; };
constexpr long long MAX_SEGMENTS = 1LL << 30;   // of a batch: the segment tables are indexed by int

static MixedSums mixed_sums(const SaisJpegHeader* hd, int n) {
    MixedSums m{};
    for (int i = 0; i < n; ++i) {
        ImgRec r{};
        if (!image_geometry(hd[i], r) || hd[i].scan_bytes <= 0 || hd[i].scan_bytes >= (1LL << 28)) continue;
        m.scan += hd[i].scan_bytes;
        m.segments += r.nseg;
        m.blocks += r.blocks;
        m.planes += plane_bytes_of(r);
        if (r.blocks > m.max_blocks) m.max_blocks = r.blocks;
        if (quads_of(r) > m.max_quads) m.max_quads = quads_of(r);
    }
    return m;
}

__constant__ unsigned char k_natural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};

struct WsPtrs {
    ImgRec* rec; int* segk; int* sego; int* sege; unsigned char* ds; unsigned long long* en; unsigned long long* ex;
    int* base; int* flags; short* coef; unsigned char* planes;
    long long coef_cap, plane_cap, nsub;
};

// What jpeg_layout holds every image against.  uniform: every header has the batch geometry and image i is slot i of
// out [n,H,W,3]; otherwise out_off is the caller's table of byte offsets into out (out_bytes long).
struct Geo {
    int uniform, max_blocks;
    long long max_quads, out_bytes;
    const long long* out_off;
};

// ---------------------------------------------------------------- layout + header checks (one thread)
__global__ void jpeg_layout(SaisJpegBatch b, const SaisJpegHeader* hd, WsPtrs w, long long ds_cap, Geo g, int* status) {
    if (threadIdx.x != 0) return;
    long long ds = 0, scan = 0, coef = 0, planes = 0;
    int sub = 0, seg = 0;
    for (int i = 0; i < b.n; ++i) {
        const SaisJpegHeader& h = hd[i];
        ImgRec r{};
        bool ok = image_geometry(h, r) && h.scan_offset >= 0 && h.scan_bytes > 0 && h.scan_bytes < (1LL << 28) &&
                  h.scan_offset + h.scan_bytes <= b.data_bytes;
        if (g.uniform) ok = ok && h.height == b.height && h.width == b.width;
        for (int c = 0; c < 3; ++c)
            ok = ok && h.qsel[c] >= 0 && h.qsel[c] < 4 && h.dcsel[c] >= 0 && h.dcsel[c] < 2 && h.acsel[c] >= 0 &&
                 h.acsel[c] < 2;
        long long cap = 0, pb = 0;
        if (ok) {
            cap = (h.scan_bytes + 2LL * SUB_BYTES * r.nseg + 2 * SUB_BYTES + SUB_BYTES - 1) / SUB_BYTES * SUB_BYTES;
            pb = plane_bytes_of(r);
            r.out_off = g.uniform ? (long long)i * b.height * b.width * 3 : g.out_off[i];
            // a header larger than the workspace or the launch grids allow, or an output outside `out`: flagged, nothing written
            ok = scan + h.scan_bytes <= b.total_scan_bytes && seg + r.nseg <= b.total_segments && ds + cap <= ds_cap &&
                 cap < (1LL << 29) && coef + r.blocks <= w.coef_cap && planes + pb <= w.plane_cap &&
                 r.blocks <= g.max_blocks && quads_of(r) <= g.max_quads && r.out_off >= 0 &&
                 r.out_off + (long long)r.H * r.W * 3 <= g.out_bytes;
        }
        r.ds_off = ds; r.sub_base = sub; r.seg_base = seg; r.coef_off = coef; r.plane_off = planes;
        if (!ok) {
            status[i] |= SAIS_JPEG_E_MARKER;
            r.nseg = 0; r.nsub = 0; r.blocks = 0;
        } else {
            r.ds_cap = (int)cap; r.nsub = (int)(cap / SUB_BYTES);
            ds += cap; sub += r.nsub; seg += r.nseg; scan += h.scan_bytes; coef += r.blocks; planes += pb;
        }
        w.rec[i] = r;
    }
}

// ---------------------------------------------------------------- destuff (one workgroup per image)
DEVINL bool is_rst(unsigned c) { return c >= 0xD0 && c <= 0xD7; }

__global__ __launch_bounds__(NT) void jpeg_destuff(SaisJpegBatch b, const unsigned char* data, const SaisJpegHeader* hd,
                                                   WsPtrs w, int* status) {
    const int img = blockIdx.x, t = threadIdx.x;
    __shared__ int s_end, s_bad, s_empty, s_k[NT], s_r[NT], s_ktot, s_rtot;
    if (status[img]) return;                                   // uniform across the workgroup
    const ImgRec r = w.rec[img];
    const unsigned char* d = data + hd[img].scan_offset;
    const long long L = hd[img].scan_bytes;
    const long long chunk = (L + NT - 1) / NT;
    const long long a = t * chunk, e = a + chunk < L ? a + chunk : L;
    if (t == 0) { s_end = (int)L; s_bad = 0; s_empty = 0; }
    __syncthreads();
    for (long long i = a; i < e; ++i) {                        // first marker that is not RSTn ends the scan
        if (d[i] == 0xFF) {
            unsigned nx = i + 1 < L ? d[i + 1] : 0x00u;
            if (i + 1 < L && nx != 0x00 && nx != 0xFF && !is_rst(nx)) { atomicMin(&s_end, (int)i); break; }
        }
    }
    __syncthreads();
    const long long end = s_end;
    if (end == L) {                                            // no marker after the scan
        if (t == 0) atomicOr(&status[img], SAIS_JPEG_E_MARKER);
        return;
    }
    const long long e2 = e < end ? e : end;
    // byte classes: keep, or RST event (the marker byte after 0xFF), or drop
    int kc = 0, rc = 0;
    for (long long i = a; i < e2; ++i) {
        unsigned c = d[i], p = i > 0 ? d[i - 1] : 0u;
        if (c == 0xFF) { kc += (i + 1 < L && d[i + 1] == 0x00); continue; }
        if (p == 0xFF) { rc += is_rst(c); continue; }
        ++kc;
    }
    s_k[t] = kc; s_r[t] = rc;
    __syncthreads();
    if (t == 0) {
        int ks = 0, rs = 0;
        for (int i = 0; i < NT; ++i) { int k = s_k[i], q = s_r[i]; s_k[i] = ks; s_r[i] = rs; ks += k; rs += q; }
        s_ktot = ks; s_rtot = rs;
    }
    __syncthreads();
    if (s_rtot + 1 != r.nseg) {                                // RSTs without DRI, or too many / too few intervals
        if (t == 0) atomicOr(&status[img], SAIS_JPEG_E_MARKER);
        return;
    }
    int* segk = w.segk + r.seg_base;
    int* sego = w.sego + r.seg_base;
    int* sege = w.sege + r.seg_base;
    {
        int k = s_k[t], s = s_r[t];
        for (long long i = a; i < e2; ++i) {
            unsigned c = d[i], p = i > 0 ? d[i - 1] : 0u;
            if (c == 0xFF) { k += (i + 1 < L && d[i + 1] == 0x00); continue; }
            if (p == 0xFF) {
                if (is_rst(c)) {
                    if (c != 0xD0u + (s & 7)) s_bad = 1;       // RST(s) opens segment s + 1
                    ++s;
                    segk[s] = k;
                }
                continue;
            }
            ++k;
        }
        if (t == 0) segk[0] = 0;
    }
    __threadfence_block();
    __syncthreads();
    if (s_bad) {
        if (t == 0) atomicOr(&status[img], SAIS_JPEG_E_MARKER);
        return;
    }
    for (int s = t; s < r.nseg; s += NT) {
        int k0 = segk[s], k1 = s + 1 < r.nseg ? segk[s + 1] : s_ktot;
        int o = (k0 + 2 * s * SUB_BYTES + SUB_BYTES - 1) / SUB_BYTES * SUB_BYTES;
        sego[s] = o;
        sege[s] = o + (k1 - k0);
        if (k1 == k0) s_empty = 1;                             // no subsequence would own the interval: nobody would miss its MCUs
    }
    __threadfence_block();
    __syncthreads();
    if (s_empty) {
        if (t == 0) atomicOr(&status[img], SAIS_JPEG_E_SHORT);
        return;
    }
    unsigned char* out = w.ds + r.ds_off;
    {
        int k = s_k[t], s = s_r[t];
        int shift = sego[s] - segk[s];
        for (long long i = a; i < e2; ++i) {
            unsigned c = d[i], p = i > 0 ? d[i - 1] : 0u;
            if (c == 0xFF) {
                if (i + 1 < L && d[i + 1] == 0x00) { out[k + shift] = 0xFF; ++k; }
                continue;
            }
            if (p == 0xFF) {
                if (is_rst(c)) { ++s; shift = sego[s] - segk[s]; }
                continue;
            }
            out[k + shift] = (unsigned char)c;
            ++k;
        }
    }
}

// ---------------------------------------------------------------- Huffman decode
struct Dec {
    const unsigned* words; int nwords;                         // the image's destuffed region, big-endian bytes
    const SaisJpegHeader* h;
    int bpm, ny, dmask, amask;                                 // table of component c: bit c of dmask / amask
};

DEVINL unsigned ld_be(const Dec& x, int wi) { return wi < x.nwords ? __builtin_bswap32(x.words[wi]) : 0u; }

DEVINL unsigned peek32(const Dec& x, unsigned pos) {
    int wi = (int)(pos >> 5), sh = (int)(pos & 31);
    unsigned a = ld_be(x, wi);
    return sh ? (a << sh) | (ld_be(x, wi + 1) >> (32 - sh)) : a;
}

constexpr unsigned long long STATE_MASK = 0xFFFFFFFFFFFFull;     // pos:32 | slot:8 | k:8; count in bits 48..63
DEVINL unsigned long long pack(unsigned pos, int c, int k) {
    return ((unsigned long long)pos << 16) | ((unsigned)c << 8) | (unsigned)k;
}

// Decodes codewords from (pos, c, k) while pos < stop and blk < blk_end; each codeword consumes >= 1 bit and the
// iteration count is bounded, so corrupt data ends the loop too.  blk: the block the next codeword belongs to.
template <bool WRITE>
DEVINL void run(const Dec& x, unsigned& pos, int& c, int& k, unsigned stop, unsigned seg_end_bits, int& blk,
                int blk_lo, int blk_end, short* coef, int& err, int& count) {
    for (int it = 0; it < 8 * SUB_BYTES + 64 && pos < stop && blk < blk_end; ++it) {
        unsigned bits = peek32(x, pos);
        const int comp = c < x.ny ? 0 : c - x.ny + 1;
        const SaisJpegHuff* t = k == 0 ? &x.h->dc[(x.dmask >> comp) & 1] : &x.h->ac[(x.amask >> comp) & 1];
        unsigned e = t->lookup[bits >> 23];
        int len = (int)(e >> 8), sym = (int)(e & 255), bad = 0;
        if (!len) {
            sym = 0;
            for (int l = 10; l <= 16; ++l) {
                int code = (int)(bits >> (32 - l));
                if (code <= t->maxcode[l]) { len = l; sym = t->huffval[(code + t->valoffset[l]) & 255]; break; }
            }
            if (!len) { len = 16; bad = SAIS_JPEG_E_CODE; }
        }
        int s = k == 0 ? sym : (sym & 15), run_ = sym >> 4;
        if (s > (k == 0 ? 11 : 10)) { bad = SAIS_JPEG_E_CODE; s = 0; }
        int v = 0;
        if (s) {
            v = (int)((bits << len) >> (32 - s));
            if (v < (1 << (s - 1))) v += 1 - (1 << s);
        }
        pos += (unsigned)(len + s);
        if (k == 0) {
            if (WRITE && blk >= blk_lo) coef[(long long)blk * 64] = (short)v;
            ++count;
            k = 1;
        } else if (s) {
            k += run_;
            if (k > 63) { bad |= SAIS_JPEG_E_RUN; k = 63; }
            if (WRITE && blk >= blk_lo) coef[(long long)blk * 64 + k_natural[k]] = (short)v;
            ++k;
        } else if (run_ == 15) {
            k = k + 16 > 64 ? 64 : k + 16;                     // ZRL past the end closes the block, as in jdhuff.c
        } else {
            k = 64;                                            // EOB
        }
        if (pos > seg_end_bits) bad |= SAIS_JPEG_E_SHORT;
        if (WRITE && blk >= blk_lo) err |= bad;
        if (k >= 64) { k = 0; c = c + 1 == x.bpm ? 0 : c + 1; ++blk; }
    }
}

struct SubInfo { int img, j, s; bool first, last, live; unsigned sub_end_bits, seg_end_bits, seg_start_bits; };

DEVINL SubInfo locate(const WsPtrs& w, int n, int g) {
    SubInfo si{};
    int lo = 0, hi = n - 1;                                    // last image with sub_base <= g
    while (lo < hi) { int m = (lo + hi + 1) >> 1; if (w.rec[m].sub_base <= g) lo = m; else hi = m - 1; }
    const ImgRec& r = w.rec[lo];
    si.img = lo;
    si.j = g - r.sub_base;
    if (si.j < 0 || si.j >= r.nsub || r.nseg == 0) return si;
    const int* sego = w.sego + r.seg_base;
    const int* sege = w.sege + r.seg_base;
    int jb = si.j * SUB_BYTES;
    int a = 0, z = r.nseg - 1;                                 // last segment with sego <= jb
    while (a < z) { int m = (a + z + 1) >> 1; if (sego[m] <= jb) a = m; else z = m - 1; }
    if (sego[a] > jb || jb >= sege[a]) return si;              // padding between segments
    si.s = a;
    si.live = true;
    si.first = jb == sego[a];
    si.last = jb + SUB_BYTES >= sege[a];
    si.sub_end_bits = (unsigned)(jb + SUB_BYTES) * 8u;
    si.seg_end_bits = (unsigned)sege[a] * 8u;
    si.seg_start_bits = (unsigned)sego[a] * 8u;
    return si;
}

DEVINL Dec make_dec(const WsPtrs& w, const SaisJpegHeader& h, const ImgRec& r) {
    Dec x;
    x.words = (const unsigned*)(w.ds + r.ds_off);
    x.nwords = r.ds_cap / 4;
    x.h = &h;
    x.bpm = r.bpm;
    x.ny = r.ny;
    x.dmask = h.dcsel[0] | h.dcsel[1] << 1 | h.dcsel[2] << 2;
    x.amask = h.acsel[0] | h.acsel[1] << 1 | h.acsel[2] << 2;
    return x;
}

// pass 0: every subsequence from a guessed state (a segment's first subsequence from its exact start)
__global__ __launch_bounds__(NT) void jpeg_sync_spec(int n, const SaisJpegHeader* hd, WsPtrs w, const int* status) {
    int g = blockIdx.x * NT + threadIdx.x;
    if (g >= w.nsub) return;
    SubInfo si = locate(w, n, g);
    if (!si.live || status[si.img]) return;
    const ImgRec& r = w.rec[si.img];
    const int gi = r.sub_base + si.j;
    Dec x = make_dec(w, hd[si.img], r);
    int blk = 0, err = 0, count = 0, c = 0, k = 0;
    unsigned pos = si.seg_start_bits;
    if (!si.first) {                                           // warm up over up to WARMUP preceding subsequences
        unsigned from = si.j * SUB_BYTES * 8u - WARMUP * SUB_BYTES * 8u;
        if (si.j * SUB_BYTES - WARMUP * SUB_BYTES > (int)(si.seg_start_bits / 8u)) pos = from;
        for (unsigned b = pos + SUB_BYTES * 8u; b <= si.j * SUB_BYTES * 8u; b += SUB_BYTES * 8u)
            run<false>(x, pos, c, k, b, si.seg_end_bits, blk, 0, 1 << 30, nullptr, err, count);
    }
    w.en[gi] = pack(pos, c, k);
    if (si.last) return;                                       // its exit state is nobody's entry
    count = 0;
    run<false>(x, pos, c, k, si.sub_end_bits, si.seg_end_bits, blk, 0, 1 << 30, nullptr, err, count);
    w.ex[gi] = pack(pos, c, k) | ((unsigned long long)count << 48);
    if (!si.first) w.flags[si.img] = 1;
}

// pass p: take the predecessor's exit as entry; re-decode if it differs from the entry used so far
__global__ __launch_bounds__(NT) void jpeg_sync_pass(int n, int p, const SaisJpegHeader* hd, WsPtrs w,
                                                     const int* status) {
    int g = blockIdx.x * NT + threadIdx.x;
    if (g >= w.nsub) return;
    SubInfo si = locate(w, n, g);
    if (!si.live || si.first || status[si.img]) return;
    if (w.flags[(p - 1) * n + si.img] == 0) return;            // converged in an earlier pass
    const ImgRec& r = w.rec[si.img];
    const int gi = r.sub_base + si.j;
    unsigned long long entry = __hip_atomic_load(&w.ex[gi - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & STATE_MASK;
    if (entry == w.en[gi]) return;
    w.en[gi] = entry;
    if (si.last) return;
    unsigned pos = (unsigned)(entry >> 16);
    int c = (int)((entry >> 8) & 255), k = (int)(entry & 255);
    if (c >= r.bpm || k >= 64) { c = 0; k = 0; }
    Dec x = make_dec(w, hd[si.img], r);
    int blk = 0, err = 0, count = 0;
    run<false>(x, pos, c, k, si.sub_end_bits, si.seg_end_bits, blk, 0, 1 << 30, nullptr, err, count);
    unsigned long long ex = pack(pos, c, k) | ((unsigned long long)count << 48);
    __hip_atomic_store(&w.ex[gi], ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w.flags[p * n + si.img] = 1;
}

// per image: base[j] = first block index started in subsequence j (segmented exclusive scan); convergence check
__global__ __launch_bounds__(NT) void jpeg_block_scan(int n, WsPtrs w, int* status) {
    const int img = blockIdx.x, t = threadIdx.x;
    __shared__ int s_carry[NT], s_reset[NT];
    if (status[img]) return;
    const ImgRec r = w.rec[img];
    if (w.flags[(MAX_PASSES - 1) * n + img]) {
        if (t == 0) atomicOr(&status[img], SAIS_JPEG_E_SYNC);
        return;
    }
    const int chunk = (r.nsub + NT - 1) / NT, a = t * chunk, e = a + chunk < r.nsub ? a + chunk : r.nsub;
    int sum = 0, reset = 0;
    for (int j = a; j < e; ++j) {
        SubInfo si = locate(w, n, r.sub_base + j);
        if (!si.live) continue;
        if (si.first) { sum = 0; reset = 1; }
        if (!si.last) sum += (int)(w.ex[r.sub_base + j] >> 48);
    }
    s_carry[t] = sum; s_reset[t] = reset;
    __syncthreads();
    if (t == 0) {
        int carry = 0;
        for (int i = 0; i < NT; ++i) { int v = s_carry[i]; s_carry[i] = carry; carry = s_reset[i] ? v : carry + v; }
    }
    __syncthreads();
    int run_ = s_carry[t];
    for (int j = a; j < e; ++j) {
        SubInfo si = locate(w, n, r.sub_base + j);
        if (!si.live) continue;
        if (si.first) run_ = 0;
        w.base[r.sub_base + j] = si.s * r.ri * r.bpm + run_;
        if (!si.last) run_ += (int)(w.ex[r.sub_base + j] >> 48);
    }
}

__global__ __launch_bounds__(NT) void jpeg_huff_write(int n, const SaisJpegHeader* hd, WsPtrs w, int* status) {
    int g = blockIdx.x * NT + threadIdx.x;
    if (g >= w.nsub) return;
    SubInfo si = locate(w, n, g);
    if (!si.live || status[si.img]) return;
    const ImgRec& r = w.rec[si.img];
    const int gi = r.sub_base + si.j;
    const int blo = r.ri ? si.s * r.ri * r.bpm : 0;
    const int bhi = r.ri && blo + r.ri * r.bpm < r.blocks ? blo + r.ri * r.bpm : r.blocks;
    unsigned long long entry = w.en[gi];
    unsigned pos = (unsigned)(entry >> 16);
    int c = (int)((entry >> 8) & 255), k = (int)(entry & 255);
    int blk = w.base[gi] - (k ? 1 : 0);
    if (blk >= bhi) return;                                    // data after the interval's last MCU: ignored
    if (c >= r.bpm || k >= 64 || blk < blo || blk % r.bpm != c) { atomicOr(&status[si.img], SAIS_JPEG_E_SYNC); return; }
    Dec x = make_dec(w, hd[si.img], r);
    short* coef = w.coef + r.coef_off * 64;
    unsigned stop = si.last ? si.seg_end_bits + 8u * SUB_BYTES : si.sub_end_bits;
    int err = 0, count = 0;
    run<true>(x, pos, c, k, stop, si.seg_end_bits, blk, blo, bhi, coef, err, count);
    if (si.last && blk < bhi) err |= SAIS_JPEG_E_SHORT;
    if (err) atomicOr(&status[si.img], err);
}

// DC prediction per (image, component): segmented prefix sum over the component's blocks in MCU order
__global__ __launch_bounds__(NT) void jpeg_dc_scan(WsPtrs w, const int* status) {
    const int img = blockIdx.x, comp = blockIdx.y, t = threadIdx.x;
    __shared__ int s_carry[NT], s_reset[NT];
    if (status[img]) return;
    const ImgRec r = w.rec[img];
    const int per = comp == 0 ? r.ny : 1, off = comp == 0 ? 0 : r.ny + comp - 1;
    const int mcus = r.mcux * r.mcuy, total = mcus * per;
    short* coef = w.coef + r.coef_off * 64;
    const int chunk = (total + NT - 1) / NT, a = t * chunk, e = a + chunk < total ? a + chunk : total;
    auto at = [&](int q) -> short* { return coef + ((long long)(q / per) * r.bpm + off + q % per) * 64; };
    auto starts = [&](int q) { return q % per == 0 && r.ri && (q / per) % r.ri == 0; };
    int sum = 0, reset = 0;
    for (int q = a; q < e; ++q) {
        if (starts(q)) { sum = 0; reset = 1; }
        sum += *at(q);
    }
    s_carry[t] = sum; s_reset[t] = reset;
    __syncthreads();
    if (t == 0) {
        int carry = 0;
        for (int i = 0; i < NT; ++i) { int v = s_carry[i]; s_carry[i] = carry; carry = s_reset[i] ? v : carry + v; }
    }
    __syncthreads();
    int acc = s_carry[t];
    for (int q = a; q < e; ++q) {
        if (starts(q)) acc = 0;
        short* p = at(q);
        acc += *p;
        *p = (short)acc;
    }
}

// ---------------------------------------------------------------- jidctint.c jpeg_idct_islow
#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

template <int SHIFT>
DEVINL void idct8(int x0, int x1, int x2, int x3, int x4, int x5, int x6, int x7, int* o) {
    int z1 = (x2 + x6) * FIX_0_541196100;
    int tmp2 = z1 - x6 * FIX_1_847759065;
    int tmp3 = z1 + x2 * FIX_0_765366865;
    int tmp0 = (x0 + x4) * (1 << 13);
    int tmp1 = (x0 - x4) * (1 << 13);
    int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    int a0 = x7, a1 = x5, a2 = x3, a3 = x1;
    int y1 = a0 + a3, y2 = a1 + a2, y3 = a0 + a2, y4 = a1 + a3;
    int z5 = (y3 + y4) * FIX_1_175875602;
    a0 *= FIX_0_298631336; a1 *= FIX_2_053119869; a2 *= FIX_3_072711026; a3 *= FIX_1_501321110;
    y1 *= -FIX_0_899976223; y2 *= -FIX_2_562915447;
    y3 = y3 * -FIX_1_961570560 + z5; y4 = y4 * -FIX_0_390180644 + z5;
    a0 += y1 + y3; a1 += y2 + y4; a2 += y2 + y3; a3 += y1 + y4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (t10 + a3 + R) >> SHIFT; o[7] = (t10 - a3 + R) >> SHIFT;
    o[1] = (t11 + a2 + R) >> SHIFT; o[6] = (t11 - a2 + R) >> SHIFT;
    o[2] = (t12 + a1 + R) >> SHIFT; o[5] = (t12 - a1 + R) >> SHIFT;
    o[3] = (t13 + a0 + R) >> SHIFT; o[4] = (t13 - a0 + R) >> SHIFT;
}

DEVINL unsigned range_limit(int v) {                           // the post-IDCT table, indexed by v & RANGE_MASK
    int x = v & 1023;
    return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}

__global__ __launch_bounds__(NT) void jpeg_idct(const SaisJpegHeader* hd, WsPtrs w, int* status) {
    const int img = blockIdx.y, b = blockIdx.x * NT + threadIdx.x;
    if (status[img]) return;
    const ImgRec& r = w.rec[img];
    if (b >= r.blocks) return;
    const int mcu = b / r.bpm, slot = b - mcu * r.bpm, mx = mcu % r.mcux, my = mcu / r.mcux;
    const int comp = slot < r.ny ? 0 : slot - r.ny + 1;
    int bx, by, stride;
    unsigned char* plane = w.planes + r.plane_off;
    if (comp == 0) { bx = mx * r.hs + slot % r.hs; by = my * r.vs + slot / r.hs; stride = r.ystride; }
    else { bx = mx; by = my; stride = r.cstride; plane += r.yplane + (comp - 1) * r.cplane; }
    const uint16_t* q = hd[img].quant[hd[img].qsel[comp]];
    const short* cp = w.coef + (r.coef_off + b) * 64;
    int d[64];
    for (int i = 0; i < 8; ++i) {
        u32x4 v = *(const u32x4*)(cp + 8 * i);
        for (int e = 0; e < 4; ++e) {
            d[8 * i + 2 * e] = (short)(v[e] & 0xFFFF) * (int)q[8 * i + 2 * e];
            d[8 * i + 2 * e + 1] = (short)(v[e] >> 16) * (int)q[8 * i + 2 * e + 1];
        }
    }
    // Encoder output keeps |coef * q| far inside int16; libjpeg-turbo's C and SIMD IDCTs can part ways beyond it (64-bit
    // vs 16-bit products), so such a block sends its image to the host decoder instead of guessing which one runs there
    int big = 0;
    for (int i = 0; i < 64; ++i) big |= d[i] > 32767 || d[i] < -32768;
    if (big) { atomicOr(&status[img], SAIS_JPEG_E_RANGE); return; }
    // The same holds past the 16-bit workspace of the SIMD column pass and past the range-limit table (row-pass output outside
    // [-512, 511]), where jidctint.c wraps (`& RANGE_MASK`) and the SIMD IDCT saturates
    int ws[64];
    for (int col = 0; col < 8; ++col) {
        int o[8];
        if (!(d[8 + col] | d[16 + col] | d[24 + col] | d[32 + col] | d[40 + col] | d[48 + col] | d[56 + col])) {
            for (int i = 0; i < 8; ++i) o[i] = d[col] * 4;
        } else {
            idct8<11>(d[col], d[8 + col], d[16 + col], d[24 + col], d[32 + col], d[40 + col], d[48 + col], d[56 + col], o);
        }
        for (int i = 0; i < 8; ++i) { ws[8 * i + col] = o[i]; big |= o[i] > 32767 || o[i] < -32768; }
    }
    unsigned char* dst = plane + (long long)(by * 8) * stride + bx * 8;
    for (int row = 0; row < 8; ++row) {
        const int* p = ws + 8 * row;
        int o[8];
        idct8<18>(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], o);
        for (int i = 0; i < 8; ++i) big |= o[i] > 511 || o[i] < -512;
        u32x2 pk;
        pk[0] = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
        pk[1] = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
        *(u32x2*)(dst + (long long)row * stride) = pk;
    }
    if (big) atomicOr(&status[img], SAIS_JPEG_E_RANGE);
}

// ---------------------------------------------------------------- fancy upsampling + ycc_rgb_convert
DEVINL int chroma(const unsigned char* p, int stride, int dw, int dh, int hs, int vs, int y, int x) {
    if (hs == 1) return p[(long long)y * stride + x];
    const int i = x >> 1;
    if (vs == 1) {
        const unsigned char* row = p + (long long)y * stride;
        int v = row[i];
        if (dw <= 2) return v;
        return x & 1 ? (3 * v + row[i + 1 < dw ? i + 1 : dw - 1] + 2) >> 2 : (3 * v + row[i > 0 ? i - 1 : 0] + 1) >> 2;
    }
    const int rr = y >> 1;
    if (dw <= 2) return p[(long long)rr * stride + i];
    const int rf = y & 1 ? (rr + 1 < dh ? rr + 1 : dh - 1) : (rr > 0 ? rr - 1 : 0);
    const unsigned char* n0 = p + (long long)rr * stride;
    const unsigned char* f0 = p + (long long)rf * stride;
    const int i2 = x & 1 ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
    int cs = 3 * n0[i] + f0[i], cn = 3 * n0[i2] + f0[i2];
    return x & 1 ? (3 * cs + cn + 7) >> 4 : (3 * cs + cn + 8) >> 4;
}

DEVINL unsigned clamp255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (unsigned)v; }

__global__ __launch_bounds__(NT) void jpeg_color(WsPtrs w, const int* status, unsigned char* out) {
    const int img = blockIdx.y;
    if (status[img]) return;
    const ImgRec& r = w.rec[img];
    const int H = r.H, W = r.W;
    const int qw = (W + 3) / 4;
    const long long gid = (long long)blockIdx.x * NT + threadIdx.x;
    if (gid >= (long long)H * qw) return;
    const int y = (int)(gid / qw), x0 = (int)(gid % qw) * 4;
    const unsigned char* yp = w.planes + r.plane_off;
    const unsigned char* cbp = yp + r.yplane;
    const unsigned char* crp = cbp + r.cplane;
    const int dw = (W + r.hs - 1) / r.hs, dh = (H + r.vs - 1) / r.vs;
    unsigned char px[12];
    const int np = W - x0 < 4 ? W - x0 : 4;
    for (int e = 0; e < np; ++e) {
        int x = x0 + e;
        int Y = yp[(long long)y * r.ystride + x];
        int cb = chroma(cbp, r.cstride, dw, dh, r.hs, r.vs, y, x) - 128;
        int cr = chroma(crp, r.cstride, dw, dh, r.hs, r.vs, y, x) - 128;
        px[3 * e] = (unsigned char)clamp255(Y + ((91881 * cr + 32768) >> 16));
        px[3 * e + 1] = (unsigned char)clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        px[3 * e + 2] = (unsigned char)clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
    unsigned char* dst = out + r.out_off + ((long long)y * W + x0) * 3;
    if (np == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned* d32 = (unsigned*)dst;
        for (int i = 0; i < 3; ++i)
            d32[i] = px[4 * i] | px[4 * i + 1] << 8 | px[4 * i + 2] << 16 | (unsigned)px[4 * i + 3] << 24;
    } else {
        for (int i = 0; i < 3 * np; ++i) dst[i] = px[i];
    }
}

// ---------------------------------------------------------------- host: marker parser
static inline int be16(const unsigned char* p) { return p[0] << 8 | p[1]; }

static int build_huff(const unsigned char* counts, const unsigned char* vals, int nvals, bool dc, SaisJpegHuff* t) {
    memset(t, 0, sizeof(*t));
    int total = 0;
    for (int l = 0; l < 16; ++l) total += counts[l];
    if (total > 256 || total > nvals) return SAIS_ERR_ARG;
    for (int i = 0; i < total; ++i) {
        if (dc && vals[i] > 15) return SAIS_JPEG_UNSUPPORTED;     // jdhuff.c rejects the table; the host decoder reports it
        t->huffval[i] = vals[i];
    }
    int code = 0, k = 0, first = 0;
    t->maxcode[0] = -1; t->maxcode[17] = -1;
    for (int l = 1; l <= 16; ++l) {
        int cnt = counts[l - 1];
        t->valoffset[l] = k - code;
        t->maxcode[l] = cnt ? code + cnt - 1 : -1;
        if (cnt && !first) first = l;
        // jpeg_make_d_derived_tbl's bogus-table test (code after length l >= 2^l), made BEFORE the lookup fill: from
        // here on code < 2^l, so every lookup index stays below 512
        if (first && code + cnt >= (1 << l)) return SAIS_JPEG_UNSUPPORTED;
        for (int i = 0; i < cnt; ++i, ++code, ++k)
            if (l <= 9)
                for (int f = 0; f < (1 << (9 - l)); ++f) t->lookup[(code << (9 - l)) | f] = (uint16_t)(l << 8 | vals[k]);
        code <<= 1;
    }
    return SAIS_OK;
}

}  // namespace

extern "C" int sais_jpeg_parse(const unsigned char* data, size_t n, SaisJpegHeader* out) {
    if (!data || !out) return SAIS_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return SAIS_ERR_ARG;
    size_t pos = 2;
    int have_sof = 0, hs[3] = {0}, vs[3] = {0}, tq[3] = {0}, id[3] = {0}, unsupported = 0;
    unsigned qdef = 0, hdef = 0;                               // bit per defined table
    uint16_t q[4][64];
    SaisJpegHuff* huff[2][4] = {{nullptr}};
    static thread_local SaisJpegHuff scratch[2][4];
    while (true) {
        if (pos + 2 > n || data[pos] != 0xFF) return SAIS_ERR_ARG;
        while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;     // fill bytes
        if (pos + 4 > n) return SAIS_ERR_ARG;
        const int m = data[pos + 1];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return SAIS_ERR_ARG;   // standalone markers before SOS
        const int len = be16(data + pos + 2);
        if (len < 2 || pos + 2 + (size_t)len > n) return SAIS_ERR_ARG;
        const unsigned char* s = data + pos + 4;
        const int sl = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof || sl < 6) return SAIS_ERR_ARG;
            have_sof = 1;
            if (s[0] != 8 || s[5] != 3) { unsupported = 1; }
            else {
                if (sl < 15) return SAIS_ERR_ARG;
                out->height = be16(s + 1);
                out->width = be16(s + 3);
                for (int c = 0; c < 3; ++c) {
                    id[c] = s[6 + 3 * c]; hs[c] = s[7 + 3 * c] >> 4; vs[c] = s[7 + 3 * c] & 15; tq[c] = s[8 + 3 * c];
                }
            }
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return SAIS_JPEG_UNSUPPORTED;                      // progressive, lossless, arithmetic, hierarchical
        } else if (m == 0xC4) {
            int o = 0;
            while (o < sl) {
                if (o + 17 > sl) return SAIS_ERR_ARG;
                int tc = s[o] >> 4, th = s[o] & 15, cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += s[o + 1 + l];
                if (tc > 1 || th > 3 || o + 17 + cnt > sl) return SAIS_ERR_ARG;
                int rc = build_huff(s + o + 1, s + o + 17, cnt, tc == 0, &scratch[tc][th]);
                if (rc == SAIS_ERR_ARG) return rc;
                if (rc) unsupported = 1;
                huff[tc][th] = &scratch[tc][th];
                hdef |= 1u << (tc * 4 + th);
                o += 17 + cnt;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < sl) {
                int pq = s[o] >> 4, t = s[o] & 15, sz = pq ? 128 : 64;
                if (pq > 1 || t > 3 || o + 1 + sz > sl) return SAIS_ERR_ARG;
                static const unsigned char zz[64] = {
                    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                    6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                    38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
                for (int i = 0; i < 64; ++i) {
                    int v = pq ? be16(s + o + 1 + 2 * i) : s[o + 1 + i];
                    if (v > 255) unsupported = 1;              // 16-bit quantisers: host decoder
                    q[t][zz[i]] = (uint16_t)v;
                }
                qdef |= 1u << t;
                o += 1 + sz;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return SAIS_ERR_ARG;
            out->restart_interval = be16(s);
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5) && s[11] == 0) unsupported = 1;   // transform 0: RGB / CMYK
        } else if (m == 0xDA) {
            if (!have_sof) return SAIS_ERR_ARG;
            if (sl < 1 || sl < 1 + 2 * s[0] + 3) return SAIS_ERR_ARG;
            if (unsupported || s[0] != 3) return SAIS_JPEG_UNSUPPORTED;
            const unsigned char* tail = s + 1 + 6;
            if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return SAIS_JPEG_UNSUPPORTED;
            if (id[0] == 'R' && id[1] == 'G' && id[2] == 'B') return SAIS_JPEG_UNSUPPORTED;
            if (!((hs[0] == 1 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 1) || (hs[0] == 2 && vs[0] == 2)) ||
                hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1)
                return SAIS_JPEG_UNSUPPORTED;
            if (out->height == 0 || out->width == 0) return SAIS_JPEG_UNSUPPORTED;   // DNL / empty
            for (int c = 0; c < 3; ++c) {
                int cs = s[1 + 2 * c], td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (cs != id[c] || td > 1 || ta > 1 || tq[c] > 3) return SAIS_JPEG_UNSUPPORTED;
                if (!(hdef >> td & 1) || !(hdef >> (4 + ta) & 1) || !(qdef >> tq[c] & 1)) return SAIS_JPEG_UNSUPPORTED;
                out->qsel[c] = tq[c]; out->dcsel[c] = td; out->acsel[c] = ta;
            }
            for (int t = 0; t < 2; ++t) {
                if (huff[0][t]) out->dc[t] = *huff[0][t];
                if (huff[1][t]) out->ac[t] = *huff[1][t];
            }
            for (int t = 0; t < 4; ++t)
                if (qdef >> t & 1) memcpy(out->quant[t], q[t], sizeof(q[t]));
            out->hsamp = hs[0]; out->vsamp = vs[0];
            int mcux = (out->width + 8 * hs[0] - 1) / (8 * hs[0]), mcuy = (out->height + 8 * vs[0] - 1) / (8 * vs[0]);
            out->mcu_count = mcux * mcuy;
            out->segments = out->restart_interval ? (out->mcu_count + out->restart_interval - 1) / out->restart_interval : 1;
            out->scan_offset = (int64_t)(pos + 2 + len);
            out->scan_bytes = (int64_t)n - out->scan_offset;
            if (out->scan_bytes < 2 || out->scan_bytes >= (1LL << 28)) return SAIS_JPEG_UNSUPPORTED;
            return SAIS_OK;
        }
        pos += 2 + (size_t)len;
    }
}

namespace {
// every phase, for a batch whose regions `L` and limits `g` the entry has fixed
int launch_decode(const SaisJpegBatch& b, const unsigned char* data, const SaisJpegHeader* headers, unsigned char* ws,
                  const Layout& L, const Geo& g, unsigned char* out, int* status, hipStream_t st) {
    WsPtrs w;
    w.rec = (ImgRec*)(ws + L.rec); w.segk = (int*)(ws + L.segk); w.sego = (int*)(ws + L.sego);
    w.sege = (int*)(ws + L.sege); w.ds = ws + L.ds; w.en = (unsigned long long*)(ws + L.en);
    w.ex = (unsigned long long*)(ws + L.ex); w.base = (int*)(ws + L.base); w.flags = (int*)(ws + L.flags);
    w.coef = (short*)(ws + L.coef); w.planes = ws + L.planes;
    w.coef_cap = L.coef_cap; w.plane_cap = L.plane_cap; w.nsub = L.nsub;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * b.n, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws + L.ds, 0, L.en - L.ds, st);              // zero gaps between segments
    if (e == hipSuccess) e = hipMemsetAsync(ws + L.flags, 0, L.planes - L.flags, st);    // pass flags + coefficients
    if (e != hipSuccess) { sais_set_last_error((int)e); return SAIS_ERR_LAUNCH; }
    hipLaunchKernelGGL(jpeg_layout, dim3(1), dim3(64), 0, st, b, headers, w, L.ds_cap, g, status);
    hipLaunchKernelGGL(jpeg_destuff, dim3(b.n), dim3(NT), 0, st, b, data, headers, w, status);
    const int gs = (int)((L.nsub + NT - 1) / NT);
    hipLaunchKernelGGL(jpeg_sync_spec, dim3(gs), dim3(NT), 0, st, b.n, headers, w, status);
    for (int p = 1; p < MAX_PASSES; ++p)
        hipLaunchKernelGGL(jpeg_sync_pass, dim3(gs), dim3(NT), 0, st, b.n, p, headers, w, status);
    hipLaunchKernelGGL(jpeg_block_scan, dim3(b.n), dim3(NT), 0, st, b.n, w, status);
    hipLaunchKernelGGL(jpeg_huff_write, dim3(gs), dim3(NT), 0, st, b.n, headers, w, status);
    hipLaunchKernelGGL(jpeg_dc_scan, dim3(b.n, 3), dim3(NT), 0, st, w, status);
    hipLaunchKernelGGL(jpeg_idct, dim3((unsigned)((g.max_blocks + NT - 1) / NT), b.n), dim3(NT), 0, st, headers, w, status);
    hipLaunchKernelGGL(jpeg_color, dim3((unsigned)((g.max_quads + NT - 1) / NT), b.n), dim3(NT), 0, st, w, status, out);
    return sais_check_launch();
}
}  // namespace

extern "C" size_t sais_jpeg_workspace_bytes(int n, int height, int width, int64_t total_scan_bytes, int total_segments) {
    if (n <= 0 || height <= 0 || width <= 0 || total_scan_bytes < 0 || total_segments < n) return 0;
    return layout_of(n, height, width, total_scan_bytes, total_segments, nullptr).total;
}

extern "C" int sais_jpeg_decode(const SaisJpegBatch* batch, const unsigned char* data, const SaisJpegHeader* headers,
                                void* workspace, size_t workspace_bytes, unsigned char* out, int* status, void* stream) {
    SAIS_ENTER();
    if (!batch || !data || !headers || !workspace || !out || !status) return SAIS_ERR_ARG;
    const SaisJpegBatch b = *batch;
    if (b.n <= 0 || b.height <= 0 || b.width <= 0 || b.total_scan_bytes <= 0 || b.total_segments < b.n ||
        b.data_bytes < b.total_scan_bytes)
        return SAIS_ERR_ARG;
    Geo g{};
    g.uniform = 1;
    const Layout L = layout_of(b.n, b.height, b.width, b.total_scan_bytes, b.total_segments, &g.max_blocks);
    if (workspace_bytes < L.total || L.nsub >= (1LL << 31) / 2) return SAIS_ERR_ARG;
    g.max_quads = (long long)b.height * ((b.width + 3) / 4);
    g.out_bytes = (long long)b.n * b.height * b.width * 3;
    return launch_decode(b, data, headers, (unsigned char*)workspace, L, g, out, status, (hipStream_t)stream);
}

extern "C" size_t sais_jpeg_mixed_workspace_bytes(const SaisJpegHeader* headers_host, int n) {
    if (!headers_host || n <= 0 || n > 65535) return 0;
    const MixedSums m = mixed_sums(headers_host, n);
    if (m.blocks == 0 || m.segments > MAX_SEGMENTS) return 0;
    return layout_sums(n, m.scan, (int)m.segments, m.blocks, m.planes).total;
}

extern "C" int sais_jpeg_decode_mixed(int n, const unsigned char* data, int64_t data_bytes, const SaisJpegHeader* headers_host,
                                      const SaisJpegHeader* headers_dev, const int64_t* out_offset_host,
                                      const int64_t* out_offset_dev, void* workspace, size_t workspace_bytes, unsigned char* out,
                                      size_t out_bytes, int* status, void* stream) {
    SAIS_ENTER();
    if (!data || !headers_host || !headers_dev || !out_offset_host || !out_offset_dev || !workspace || !out || !status)
        return SAIS_ERR_ARG;
    if (n <= 0 || n > 65535 || data_bytes <= 0 || out_bytes == 0 || out_bytes >= (1ULL << 62)) return SAIS_ERR_ARG;
    const MixedSums m = mixed_sums(headers_host, n);
    if (m.blocks == 0 || m.scan > data_bytes || m.segments > MAX_SEGMENTS) return SAIS_ERR_ARG;
    for (int i = 0; i < n; ++i) {                              // the caller's offsets, on the host copy
        ImgRec r{};
        if (!image_geometry(headers_host[i], r)) continue;     // flagged on the device, writes nothing
        const long long o = out_offset_host[i];
        if (o < 0 || (unsigned long long)o + (unsigned long long)r.H * r.W * 3 > out_bytes) return SAIS_ERR_ARG;
    }
    const Layout L = layout_sums(n, m.scan, (int)m.segments, m.blocks, m.planes);
    if (workspace_bytes < L.total || L.nsub >= (1LL << 31) / 2) return SAIS_ERR_ARG;
    SaisJpegBatch b{};
    b.n = n; b.total_segments = (int)m.segments; b.total_scan_bytes = m.scan; b.data_bytes = data_bytes;
    Geo g{};
    g.max_blocks = m.max_blocks; g.max_quads = m.max_quads; g.out_bytes = (long long)out_bytes;
    g.out_off = (const long long*)out_offset_dev;
    return launch_decode(b, data, headers_dev, (unsigned char*)workspace, L, g, out, status, (hipStream_t)stream);
}
