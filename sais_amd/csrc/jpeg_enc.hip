// Baseline JPEG encode on gfx950: uint8 RGB frames on the device -> the entropy-coded scan + EOI that Pillow / libjpeg-turbo write
// at their defaults (jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c quantize, jchuff.c with the
// Annex K tables), byte for byte.  tests/jpeg_enc_ref.py restates every rule in numpy.
//
// Phases (one stable kernel name each); a block JOB is one 8 x 8 block position of the interleaved scan, dummies included:
//   jpeg_enc_dct     one wave per job: gather with clamped addresses, colour, 2 x 2 downsample, forward DCT, quantise -> int16
//                    coefficients in zigzag order
//   jpeg_enc_len     one wave per job: lane k codes coefficient k (its run from a ballot of the non-zeros) -> bits of the job
//   jpeg_enc_scan    per image: exclusive scan of the job lengths (also of the 0xFF counts per chunk, below)
//   jpeg_enc_zero    zero the words of the unstuffed stream the image will use
//   jpeg_enc_bits    one wave per job: the same codes again, assembled in LDS at the job's bit offset and written to the unstuffed
//                    stream; a word shared by two jobs is ORed into the zeroed memory, every other word has one owner
//   jpeg_enc_ffcount per 2 KiB chunk of the unstuffed stream (1-bit padding applied): its 0xFF bytes
//   jpeg_enc_stuff   write the stuffed bytes, FF D9 and nbytes; an image that does not fit out_stride gets nbytes = -1 and no byte
// The unstuffed stream is a string of bits, MSB first, kept in 32-bit words: bit p is bit 31 - p % 32 of word p / 32.
#include "common.hpp"
#include "../../include/sais_hip.h"
#include <string.h>
#include <algorithm>

namespace {

constexpr int NT = 256;                   // threads per workgroup everywhere; 4 jobs per workgroup in the wave-per-job kernels
constexpr int CHUNK = 2048;               // bytes of unstuffed stream per workgroup of the stuffing kernels: 8 per thread
constexpr int JOB_WORDS = 64;             // LDS words per job: the longest job (1658 bits) + a 31-bit shift is 53 words

// ---- Annex K Huffman tables -> (code, length) per symbol, at compile time -----------------------------------------------------
struct Spec { unsigned char counts[16]; unsigned char sym[162]; };
constexpr Spec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr Spec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr Spec AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr Spec AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code[t][sym]: (Huffman code << 8) | length, 0 = no such symbol.  t: 0 DC luma, 1 DC chroma, 2 AC luma, 3 AC chroma
struct Tables { unsigned int code[4][256]; };
constexpr void derive(const Spec& s, unsigned int* out) {
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.counts[len - 1]; ++i) out[s.sym[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
}
constexpr Tables make_tables() {
    Tables t{};
    derive(DC_LUMA, t.code[0]); derive(DC_CHROMA, t.code[1]); derive(AC_LUMA, t.code[2]); derive(AC_CHROMA, t.code[3]);
    return t;
}
constexpr Tables H_TABLES = make_tables();
__constant__ Tables D_TABLES = make_tables();

// the longest code of one block under table pair t (0 luma, 1 chroma): the longest DC code + value bits, and 63 times the longest
// AC code + value bits (a ZRL spends 11 bits on 16 coefficients: less than 16 coded coefficients)
constexpr int max_block_bits(int t) {
    int dc = 0, ac = 0;
    for (int s = 0; s < 12; ++s) {
        const int len = (int)(H_TABLES.code[t][s] & 0xff);
        if (len && len + s > dc) dc = len + s;
    }
    for (int s = 0; s < 256; ++s) {
        const int len = (int)(H_TABLES.code[2 + t][s] & 0xff);
        if (len && len + (s & 15) > ac) ac = len + (s & 15);
    }
    return dc + 63 * ac;
}
constexpr int MAX_BITS_LUMA = max_block_bits(0), MAX_BITS_CHROMA = max_block_bits(1);
static_assert((MAX_BITS_LUMA + 31 + 31) / 32 <= JOB_WORDS && (MAX_BITS_CHROMA + 31 + 31) / 32 <= JOB_WORDS, "JOB_WORDS too small");

__constant__ unsigned char D_ZIGZAG[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- geometry ----------------------------------------------------------------------------------------------------------------
struct Geo {
    int n, H, W, sub;                     // sub: 0 = 4:4:4, 2 = 4:2:0
    int mcux, mcuy, bpm;                  // MCUs per row / column, block jobs per MCU
    int wb, hb;                           // real luma blocks per row / column
    int jobs;                             // block jobs per image
    long long cap_words;                  // words of one image's unstuffed stream (worst case + 2)
    int chunks;                           // CHUNK-byte chunks of that capacity
};

struct Ws {
    short* coef;                          // [n][jobs][64]
    unsigned int* blen;                   // [n][jobs]
    unsigned long long* boff;             // [n][jobs]
    unsigned long long* total_bits;       // [n]
    unsigned int* bits;                   // [n][cap_words]
    unsigned int* ffcnt;                  // [n][chunks]
    unsigned long long* ffoff;            // [n][chunks]
    unsigned long long* fftotal;          // [n]
};

struct Layout { size_t coef, blen, boff, total_bits, bits, ffcnt, ffoff, fftotal, total; };

struct QTables { unsigned short q[2][64]; };      // natural order; a kernel argument

static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

static bool geo_of(int n, int H, int W, int sub, Geo& g) {
    if (n <= 0 || n > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || (sub != 0 && sub != 2)) return false;
    const int m = sub == 2 ? 16 : 8;
    g.n = n; g.H = H; g.W = W; g.sub = sub;
    g.mcux = (W + m - 1) / m; g.mcuy = (H + m - 1) / m; g.bpm = sub == 2 ? 6 : 3;
    g.wb = (W + 7) / 8; g.hb = (H + 7) / 8;
    const long long mcus = (long long)g.mcux * g.mcuy, jobs = mcus * g.bpm;
    if (jobs * n >= (1LL << 31) - NT) return false;                   // job indices are ints
    g.jobs = (int)jobs;
    const long long bits = mcus * ((sub == 2 ? 4 : 1) * (long long)MAX_BITS_LUMA + 2LL * MAX_BITS_CHROMA);
    g.cap_words = (bits + 31) / 32 + 2;
    const long long chunks = (g.cap_words * 4 + CHUNK - 1) / CHUNK;
    if (chunks >= (1LL << 31) / NT) return false;
    g.chunks = (int)chunks;
    return true;
}

static Layout layout_of(const Geo& g) {
    Layout L{};
    const size_t n = (size_t)g.n, jobs = (size_t)g.jobs;
    size_t o = 0;
    L.coef = o;        o = al(o + 128 * jobs * n);
    L.blen = o;        o = al(o + 4 * jobs * n);
    L.boff = o;        o = al(o + 8 * jobs * n);
    L.total_bits = o;  o = al(o + 8 * n);
    L.bits = o;        o = al(o + 4 * (size_t)g.cap_words * n);
    L.ffcnt = o;       o = al(o + 4 * (size_t)g.chunks * n);
    L.ffoff = o;       o = al(o + 8 * (size_t)g.chunks * n);
    L.fftotal = o;     o = al(o + 8 * n);
    L.total = o;
    return L;
}

// job j of an image -> component, block coordinates in the component, and whether the position is outside its real blocks
struct Job { int comp, bx, by; bool dummy; };
DEVINL Job job_of(const Geo& g, int j) {
    Job b;
    const int mcu = j / g.bpm, s = j - mcu * g.bpm;
    const int my = mcu / g.mcux, mx = mcu - my * g.mcux;
    if (g.sub == 2 && s < 4) {
        b.comp = 0; b.bx = 2 * mx + (s & 1); b.by = 2 * my + (s >> 1);
        b.dummy = b.bx >= g.wb || b.by >= g.hb;
    } else {
        b.comp = g.sub == 2 ? s - 3 : s; b.bx = mx; b.by = my; b.dummy = false;
    }
    return b;
}

// the DC of the previous real block of job j's component in scan order (0 before the first)
DEVINL int dc_predictor(const Geo& g, const short* coef, int j, const Job& b) {
    if (g.sub == 2 && b.comp == 0) {
        for (int p = j - 1; p >= 0; --p) {
            const Job o = job_of(g, p);
            if (o.comp == 0 && !o.dummy) return coef[(size_t)p * 64];
        }
        return 0;
    }
    return j >= g.bpm ? coef[(size_t)(j - g.bpm) * 64] : 0;
}

// ---- colour, DCT ---------------------------------------------------------------------------------------------------------------
DEVINL int component_of(const unsigned char* px, int comp) {
    const int r = px[0], g = px[1], b = px[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

DEVINL int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one pass over eight values; FIRST: the row pass (results scaled up by 4), else the column pass
template <bool FIRST>
DEVINL void fdct8(const int* d, int* o) {
    constexpr int N = FIRST ? 11 : 15;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { o[0] = (t10 + t11) * 4; o[4] = (t10 - t11) * 4; }
    else { o[0] = descale(t10 + t11, 2); o[4] = descale(t10 - t11, 2); }
    int z1 = (t12 + t13) * 4433;
    o[2] = descale(z1 + t13 * 6270, N);
    o[6] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    o[7] = descale(t4 + z1 + z3, N);
    o[5] = descale(t5 + z2 + z4, N);
    o[3] = descale(t6 + z2 + z3, N);
    o[1] = descale(t7 + z1 + z4, N);
}

__global__ __launch_bounds__(NT) void jpeg_enc_dct(Geo g, const unsigned char* __restrict__ rgb, QTables qt, Ws w) {
    __shared__ int tile[NT / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gj = (long long)blockIdx.x * (NT / 64) + wave;    // job over the whole batch
    const bool live = gj < (long long)g.n * g.jobs;
    const int img = live ? (int)(gj / g.jobs) : 0, j = live ? (int)(gj - (long long)img * g.jobs) : 0;
    const Job b = job_of(g, j);
    const int r = lane >> 3, c = lane & 7;
    const unsigned char* src = rgb + (size_t)img * g.H * g.W * 3;
    int v = 0;
    if (live && !b.dummy) {
        if (g.sub == 2 && b.comp > 0) {
            const int ch = (g.H + 1) / 2;
            const int cy = min(b.by * 8 + r, ch - 1), cx = b.bx * 8 + c;          // rows past ch - 1 repeat downsampled row ch - 1
            const int y0 = min(2 * cy, g.H - 1), y1 = min(2 * cy + 1, g.H - 1);
            const int x0 = min(2 * cx, g.W - 1), x1 = min(2 * cx + 1, g.W - 1);
            v = component_of(src + ((size_t)y0 * g.W + x0) * 3, b.comp) + component_of(src + ((size_t)y0 * g.W + x1) * 3, b.comp) +
                component_of(src + ((size_t)y1 * g.W + x0) * 3, b.comp) + component_of(src + ((size_t)y1 * g.W + x1) * 3, b.comp);
            v = (v + 1 + (cx & 1)) >> 2;
        } else {
            const int y = min(b.by * 8 + r, g.H - 1), x = min(b.bx * 8 + c, g.W - 1);
            v = component_of(src + ((size_t)y * g.W + x) * 3, b.comp);
        }
        v -= 128;
    }
    int* t = tile[wave];
    int d[8], o[8];
    t[lane] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = t[r * 8 + i];
    fdct8<true>(d, o);
    __syncthreads();
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) t[r * 8 + i] = o[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = t[i * 8 + c];
    fdct8<false>(d, o);
    __syncthreads();
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i * 8 + c] = o[i];
    }
    __syncthreads();
    const int nat = D_ZIGZAG[lane];
    const int x = t[nat];
    const int qv = (int)qt.q[b.comp > 0][nat] << 3;
    const int a = (abs(x) + (qv >> 1)) / qv;
    if (live) w.coef[((size_t)img * g.jobs + j) * 64 + lane] = (short)(b.dummy ? 0 : (x < 0 ? -a : a));
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------
DEVINL void append(unsigned long long& bits, int& nb, unsigned int code_len) {
    const int len = (int)(code_len & 0xff);
    bits = (bits << len) | (code_len >> 8);
    nb += len;
}

// what lane k writes for coefficient k of a job: up to three ZRL codes + the (run, size) code + the value bits (at most 59 bits);
// lane 0 the DC difference; lane 63 the EOB when coefficient 63 is zero
DEVINL void lane_code(int k, int v, int dc_diff, unsigned long long nz, int t, unsigned long long& bits, int& nb) {
    bits = 0; nb = 0;
    if (k == 0) v = dc_diff;
    const int a = abs(v), size = a ? 32 - __clz(a) : 0;
    const unsigned int val = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    if (k == 0) {
        append(bits, nb, D_TABLES.code[t][size & 0xff]);
    } else if (v != 0) {
        const unsigned long long before = nz & ((1ULL << k) - 1ULL);              // non-zero AC coefficients below k
        const int prev = before ? 63 - __clzll((long long)before) : 0;
        const int run = k - 1 - prev;
        for (int z = run >> 4; z > 0; --z) append(bits, nb, D_TABLES.code[2 + t][0xF0]);
        append(bits, nb, D_TABLES.code[2 + t][(((run & 15) << 4) | size) & 0xff]);
    } else {
        if (k == 63) append(bits, nb, D_TABLES.code[2 + t][0x00]);
        return;
    }
    bits = (bits << size) | val;
    nb += size;
}

DEVINL int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// the codes of one job: every lane's bits, their count and the exclusive prefix of the counts; returns the job's total
DEVINL int job_codes(const Geo& g, const Ws& w, int img, int j, int lane, unsigned long long& bits, int& nb, int& before) {
    const short* coef = w.coef + (size_t)img * g.jobs * 64;
    const Job b = job_of(g, j);
    const int v = coef[(size_t)j * 64 + lane];
    const unsigned long long nz = __ballot(v != 0 && lane > 0);
    int diff = 0;
    if (lane == 0 && !b.dummy) diff = v - dc_predictor(g, coef, j, b);
    lane_code(lane, v, diff, nz, b.comp > 0, bits, nb);
    const int incl = wave_incl_scan(nb, lane);
    before = incl - nb;
    return __shfl(incl, 63);
}

__global__ __launch_bounds__(NT) void jpeg_enc_len(Geo g, Ws w) {
    const int lane = threadIdx.x & 63;
    const long long gj = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (gj >= (long long)g.n * g.jobs) return;                        // whole waves leave
    const int img = (int)(gj / g.jobs), j = (int)(gj - (long long)img * g.jobs);
    unsigned long long bits;
    int nb, before;
    const int total = job_codes(g, w, img, j, lane, bits, nb, before);
    if (lane == 0) w.blen[gj] = (unsigned)total;
}

// one workgroup per image: off[i] = sum of len[0 .. i), total = the whole sum
__global__ __launch_bounds__(NT) void jpeg_enc_scan(const unsigned int* __restrict__ len, unsigned long long* __restrict__ off,
                                                    unsigned long long* __restrict__ total, int count) {
    __shared__ unsigned long long part[NT];
    const int img = blockIdx.x, t = threadIdx.x;
    len += (size_t)img * count; off += (size_t)img * count;
    const int per = (count + NT - 1) / NT, lo = min(t * per, count), hi = min(lo + per, count);
    unsigned long long s = 0;
    for (int i = lo; i < hi; ++i) s += len[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < NT; ++i) { const unsigned long long p = part[i]; part[i] = run; run += p; }
        total[img] = run;
    }
    __syncthreads();
    s = part[t];
    for (int i = lo; i < hi; ++i) { off[i] = s; s += len[i]; }
}

__global__ __launch_bounds__(NT) void jpeg_enc_zero(Geo g, Ws w) {
    const int img = blockIdx.y;
    const long long words = min((long long)((w.total_bits[img] + 31) / 32) + 1, g.cap_words);
    unsigned int* dst = w.bits + (size_t)img * g.cap_words;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < words; i += (long long)gridDim.x * NT) dst[i] = 0u;
}

__global__ __launch_bounds__(NT) void jpeg_enc_bits(Geo g, Ws w) {
    __shared__ unsigned int buf[NT / 64][JOB_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gj = (long long)blockIdx.x * (NT / 64) + wave;
    const bool live = gj < (long long)g.n * g.jobs;
    const int img = live ? (int)(gj / g.jobs) : 0, j = live ? (int)(gj - (long long)img * g.jobs) : 0;
    unsigned long long bits;
    int nb, before;
    const int total = job_codes(g, w, img, j, lane, bits, nb, before);
    const unsigned long long start = w.boff[(size_t)img * g.jobs + j];
    unsigned int* lds = buf[wave];
    lds[lane] = 0u;                                                   // JOB_WORDS == 64 lanes
    __syncthreads();
    if (live && nb > 0) {
        const int p = (int)(start & 31) + before, w0 = p >> 5, r = p & 31;       // place nb bits at bit r of word w0, MSB first
        unsigned long long x;                                         // the first 64 bits of the window
        unsigned int tail = 0;                                        // the next 32
        if (r + nb <= 64) {
            x = bits << (64 - r - nb);
        } else {
            const int sh = r + nb - 64;
            x = bits >> sh;
            tail = (unsigned)(bits & ((1ULL << sh) - 1ULL)) << (32 - sh);
        }
        const unsigned int hi = (unsigned)(x >> 32), lo = (unsigned)x;
        if (hi && w0 < JOB_WORDS) atomicOr(&lds[w0], hi);
        if (lo && w0 + 1 < JOB_WORDS) atomicOr(&lds[w0 + 1], lo);
        if (tail && w0 + 2 < JOB_WORDS) atomicOr(&lds[w0 + 2], tail);
    }
    __syncthreads();
    if (live) {
        const long long first = (long long)(start >> 5), last = (long long)((start + total - 1) >> 5);
        const int nwords = (int)(last - first) + 1;
        unsigned int* dst = w.bits + (size_t)img * g.cap_words;
        if (lane < nwords && lane < JOB_WORDS && first + lane < g.cap_words) {
            const unsigned int word = lds[lane];
            if (lane == 0 || lane == nwords - 1) { if (word) atomicOr(&dst[first + lane], word); }   // shared with a neighbour job
            else dst[first + lane] = word;
        }
    }
}

// ---- byte stuffing -------------------------------------------------------------------------------------------------------------
// byte i of an image's unstuffed stream of nbits bits; the last byte is filled up with 1-bits
DEVINL unsigned int stream_byte(const unsigned int* words, long long i, unsigned long long nbits) {
    unsigned int b = (words[i >> 2] >> (24 - 8 * (int)(i & 3))) & 0xffu;
    if ((unsigned long long)i == (nbits - 1) >> 3) b |= 0xffu >> (((nbits - 1) & 7) + 1);
    return b;
}

__global__ __launch_bounds__(NT) void jpeg_enc_ffcount(Geo g, Ws w) {
    __shared__ int wsum[NT / 64];
    const int img = blockIdx.y, t = threadIdx.x;
    const unsigned long long nbits = w.total_bits[img];
    const long long nbytes = (long long)((nbits + 7) >> 3);
    const long long base = (long long)blockIdx.x * CHUNK;
    if (base >= nbytes) {                                             // the whole workgroup: a chunk past the stream
        if (t == 0) w.ffcnt[(size_t)img * g.chunks + blockIdx.x] = 0u;
        return;
    }
    const unsigned int* words = w.bits + (size_t)img * g.cap_words;
    int cnt = 0;
    for (int e = 0; e < 8; ++e) {
        const long long i = base + t * 8 + e;
        if (i < nbytes) cnt += stream_byte(words, i, nbits) == 0xffu;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((t & 63) == 0) wsum[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) w.ffcnt[(size_t)img * g.chunks + blockIdx.x] = (unsigned)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(NT) void jpeg_enc_stuff(Geo g, Ws w, unsigned char* __restrict__ out, unsigned long long out_stride,
                                                     int* __restrict__ nbytes_out) {
    __shared__ int wsum[NT / 64];
    const int img = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const unsigned long long nbits = w.total_bits[img];
    const long long nbytes = (long long)((nbits + 7) >> 3);
    const unsigned long long file = (unsigned long long)nbytes + w.fftotal[img] + 2ULL;        // stuffed bytes + FF D9
    const bool fits = file <= out_stride && file < (1ULL << 31);
    if (blockIdx.x == 0 && t == 0) nbytes_out[img] = fits ? (int)file : -1;
    const long long base = (long long)blockIdx.x * CHUNK;
    if (!fits || base >= nbytes) return;                              // the whole workgroup
    const unsigned int* words = w.bits + (size_t)img * g.cap_words;
    unsigned int b[8];
    int cnt = 0;
    for (int e = 0; e < 8; ++e) {
        const long long i = base + t * 8 + e;
        b[e] = i < nbytes ? stream_byte(words, i, nbits) : 0u;
        cnt += b[e] == 0xffu;
    }
    const int incl = wave_incl_scan(cnt, lane);
    if (lane == 63) wsum[t >> 6] = incl;
    __syncthreads();
    int before = incl - cnt;
    for (int q = 0; q < (t >> 6); ++q) before += wsum[q];
    unsigned char* dst = out + (size_t)img * out_stride;
    unsigned long long o = (unsigned long long)(base + t * 8) + w.ffoff[(size_t)img * g.chunks + blockIdx.x] + (unsigned)before;
    for (int e = 0; e < 8; ++e) {
        const long long i = base + t * 8 + e;
        if (i >= nbytes) break;
        dst[o++] = (unsigned char)b[e];
        if (b[e] == 0xffu) dst[o++] = 0;
        if (i == nbytes - 1) { dst[o] = 0xff; dst[o + 1] = 0xd9; }
    }
}

}  // namespace

extern "C" size_t sais_jpeg_encode_bound(int height, int width, int subsampling) {
    Geo g;
    if (!geo_of(1, height, width, subsampling, g)) return 0;
    const unsigned long long mcus = (unsigned long long)g.mcux * g.mcuy;
    const unsigned long long bits = mcus * ((subsampling == 2 ? 4 : 1) * (unsigned long long)MAX_BITS_LUMA + 2ULL * MAX_BITS_CHROMA);
    return (size_t)(2 * ((bits + 7) / 8 + 1) + 2);                    // every byte stuffed, the padding byte too, + FF D9
}

extern "C" size_t sais_jpeg_encode_workspace_bytes(int n, int height, int width, int subsampling) {
    Geo g;
    if (!geo_of(n, height, width, subsampling, g)) return 0;
    return layout_of(g).total;
}

extern "C" int sais_jpeg_encode(const unsigned char* rgb, int n, int height, int width, const SaisJpegEncParams* p, void* workspace,
                                size_t workspace_bytes, unsigned char* out, size_t out_stride, int* nbytes, void* stream) {
    SAIS_ENTER();
    if (!rgb || !p || !workspace || !out || !nbytes || out_stride < 2) return SAIS_ERR_ARG;
    Geo g;
    if (!geo_of(n, height, width, p->subsampling, g)) return SAIS_ERR_ARG;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k)
            if (p->q[t][k] < 1 || p->q[t][k] > 255) return SAIS_ERR_ARG;
    const Layout L = layout_of(g);
    if (workspace_bytes < L.total) return SAIS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace;
    Ws w;
    w.coef = (short*)(ws + L.coef); w.blen = (unsigned int*)(ws + L.blen); w.boff = (unsigned long long*)(ws + L.boff);
    w.total_bits = (unsigned long long*)(ws + L.total_bits); w.bits = (unsigned int*)(ws + L.bits);
    w.ffcnt = (unsigned int*)(ws + L.ffcnt); w.ffoff = (unsigned long long*)(ws + L.ffoff);
    w.fftotal = (unsigned long long*)(ws + L.fftotal);
    QTables qt;
    memcpy(qt.q, p->q, sizeof(qt.q));
    const long long all = (long long)g.n * g.jobs;
    const unsigned job_grid = (unsigned)((all + NT / 64 - 1) / (NT / 64));
    hipLaunchKernelGGL(jpeg_enc_dct, dim3(job_grid), dim3(NT), 0, st, g, rgb, qt, w);
    hipLaunchKernelGGL(jpeg_enc_len, dim3(job_grid), dim3(NT), 0, st, g, w);
    hipLaunchKernelGGL(jpeg_enc_scan, dim3(g.n), dim3(NT), 0, st, w.blen, w.boff, w.total_bits, g.jobs);
    const unsigned zero_grid = (unsigned)std::min<long long>(1024, (g.cap_words + NT - 1) / NT);
    hipLaunchKernelGGL(jpeg_enc_zero, dim3(zero_grid, g.n), dim3(NT), 0, st, g, w);
    hipLaunchKernelGGL(jpeg_enc_bits, dim3(job_grid), dim3(NT), 0, st, g, w);
    hipLaunchKernelGGL(jpeg_enc_ffcount, dim3(g.chunks, g.n), dim3(NT), 0, st, g, w);
    hipLaunchKernelGGL(jpeg_enc_scan, dim3(g.n), dim3(NT), 0, st, w.ffcnt, w.ffoff, w.fftotal, g.chunks);
    hipLaunchKernelGGL(jpeg_enc_stuff, dim3(g.chunks, g.n), dim3(NT), 0, st, g, w, out, (unsigned long long)out_stride, nbytes);
    return sais_check_launch();
}
