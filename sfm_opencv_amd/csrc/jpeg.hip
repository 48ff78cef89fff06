// jpeg.hip -- baseline JPEG decoding on the device: entropy stage to BGR pixels (gfx950).
//
// The definition is the host decoder of sfm_opencv_amd/host/sfm_jpeg.hpp (decode_jpeg), which this file includes: one header parser
// (parse_headers), one host entropy decoder (decode_scan), one text of the inverse DCT's 1-D pass (idct_1d, host and device) and one
// place where the colour tables are rounded (ycc_tables).  Everything is integer arithmetic, so the contract is the host's bytes.
//
//   host      parse_headers; the restart markers of the scan located (jpeg_segments); tables, segment offsets and scan bytes uploaded
//   kernel 1  jpeg_huffman_kernel: one lane per restart interval -> quantised coefficients, int16, 64 per block in natural order
//             (or, for files without enough intervals, decode_scan on the host with a sink that writes the same layout)
//   kernel 2  jpeg_idct_kernel: dequantise, column pass, row pass, clamp -> the padded component planes; eight lanes per block
//   kernel 3  jpeg_colour_kernel: chroma sample by the closed form of upsample(), YCbCr tables -> BGR (or the gray plane copied)
//
// Segments.  The DC predictors are reset at every RSTn, so the intervals are independent.  Segment k starts after the k-th byte pair
// FF D0..D7 counted from the scan's start (segment 0: at the scan's start) and ends at the next such pair or at the end of the buffer;
// inside it the bit reader stops at the first FF that is not followed by 00 and feeds zeros from there.  That is what the host reader
// does: BitReader::fill never advances past an unstuffed FF, so its read pointer never passes an RSTn pair, and at each restart
// decode_scan looks from that pointer for the next pair -- which is therefore the k-th of the scan.  A file with fewer pairs than
// intervals - 1 is refused here as there.
#include "common.hpp"
#include "../host/sfm_jpeg.hpp"

namespace {

using sfm::jpeg::Frame;
using sfm::jpeg::Huff;

// the Huffman kernel's LDS: the tables of Huff as decode_symbol reads them, four DC then four AC, then the zigzag order
constexpr int JPEG_HUFF_TABLES = 8;
constexpr int JPEG_HUFF_TABLE_BYTES = 512 * 2 + (17 + 18 + 17) * 4 + 256;
constexpr int JPEG_HUFF_LDS_BYTES = JPEG_HUFF_TABLES * JPEG_HUFF_TABLE_BYTES + 64;
struct JpegHuffDev { uint16_t look[512]; int mincode[17]; int maxcode[18]; int valptr[17]; uint8_t vals[256]; };
static_assert(sizeof(JpegHuffDev) == JPEG_HUFF_TABLE_BYTES, "JpegHuffDev is packed");
// the parameter block behind them
constexpr int JPEG_QT_BYTES = 4 * 64 * 2, JPEG_YCC_BYTES = 4 * 256 * 4;
constexpr size_t JPEG_OFF_QT = JPEG_HUFF_LDS_BYTES, JPEG_OFF_YCC = JPEG_OFF_QT + JPEG_QT_BYTES, JPEG_OFF_SEG = JPEG_OFF_YCC + JPEG_YCC_BYTES;

// One lane per interval, and one interval per 64-lane workgroup (one wave): all 64 lanes load the tables and zero-fill the interval's
// blocks, then lane 0 decodes.  Lanes that decode different intervals are on different control paths nearly all the time (fast or slow
// symbol path, bytes to refill, run lengths), and a wave executes those one after the other: with 16 decoding lanes per wave the
// kernel took 16 times a single lane's time per block whatever the number of intervals (12.9 ms at 171 intervals, 0.30 ms at 9747, both
// 9 - 10 us per block and lane; profiles/r18_time_jpeg.log).  The device has 1024 SIMDs to spread the waves over.
constexpr int JPEG_HUFF_LANES = 64, JPEG_HUFF_INTERVALS = 1;
constexpr int JPEG_HUFF_STRIDE = JPEG_HUFF_LANES / JPEG_HUFF_INTERVALS;      // every STRIDE-th lane decodes
constexpr int JPEG_IDCT_BLOCKS = 32;            // blocks per 256-lane workgroup of the IDCT kernel
constexpr int JPEG_WS_ROW = 9, JPEG_WS_BLOCK = 72;      // workspace strides in words: both passes then touch each LDS bank once per wave
constexpr int JPEG_RUN = 4;                     // pixels per lane of the colour kernel

// status bits of the Huffman kernel: the conditions decode_scan treats as corrupt
enum { JPEG_BAD_DC_CATEGORY = 1, JPEG_BAD_PREDICTOR = 2, JPEG_BAD_RUN = 4, JPEG_BAD_AC_CATEGORY = 8 };

struct JpegComp {
    int h, v, tq, td, ta;
    int w, hgt, pw, ph;         // true and padded plane size
    int bw;                     // blocks per block row (pw / 8)
    unsigned blk0;              // first block of the component in the coefficient array
    unsigned plane0;            // byte offset of its plane
};
struct JpegGeom {
    int W, H, ncomp, hmax, vmax, mcux, mcuy;
    int ri;                     // MCUs per interval (all of them in a file without DRI)
    int n_int, nmcu, bpm;       // intervals, MCUs, blocks per MCU
    JpegComp c[3];
};

// block index of the j-th block of MCU `mcu` in scan order
__device__ inline unsigned jpeg_block_of(const JpegGeom& G, int mcu, int j)
{
    const int my = mcu / G.mcux, mx = mcu - my * G.mcux;
    unsigned b = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= G.ncomp) break;
        const int nb = G.c[c].h * G.c[c].v;
        if (j >= 0 && j < nb) { const int by = j / G.c[c].h, bx = j - by * G.c[c].h; b = G.c[c].blk0 + (unsigned)(my * G.c[c].v + by) * (unsigned)G.c[c].bw + (unsigned)(mx * G.c[c].h + bx); }
        j -= nb;
    }
    return b;
}

// BitReader of sfm_jpeg.hpp over [p, e) of the uploaded scan: e is the segment's end, and moves to the read position at the first
// unstuffed FF (hit_marker), so that every later byte is a zero.  No byte outside [0, e) is used.  The bytes come through a window of
// 16 (a lane's loads are a dependent chain: one global load per 16 bytes instead of one per byte); the window's load stays inside the
// scan's block, which is allocated in whole windows.
struct JpegBits {
    const uint4* s; uint32_t p, e; uint32_t acc; int n;
    uint32_t wi; uint64_t lo, hi;               // the window: bytes [16 wi, 16 wi + 16)
    __device__ uint32_t byte(uint32_t q)
    {
        const uint32_t i = q >> 4;
        if (i != wi) { const uint4 w = s[i]; lo = w.x | ((uint64_t)w.y << 32); hi = w.z | ((uint64_t)w.w << 32); wi = i; }
        return (uint32_t)(((q & 8) ? hi : lo) >> (8 * (q & 7))) & 255u;
    }
    __device__ void fill()
    {
        while (n <= 24) {
            uint32_t b = 0;
            if (p < e) {
                b = byte(p);
                if (b == 0xFF) {
                    if (p + 1 < e && byte(p + 1) == 0x00) p += 2;
                    else { e = p; b = 0; }
                } else ++p;
            }
            acc |= b << (24 - n);
            n += 8;
        }
    }
    __device__ int peek(int k) { if (n < k) fill(); return (int)(acc >> (32 - k)); }
    __device__ void skip(int k) { acc <<= k; n -= k; }
    __device__ int get(int k) { if (k == 0) return 0; const int v = peek(k); skip(k); return v; }
};

__device__ inline int jpeg_decode_symbol(JpegBits& br, const JpegHuffDev& h)
{
    const int pre = br.peek(9);
    const int e = h.look[pre];
    if (e) { br.skip(e >> 8); return e & 255; }
    const int code = br.peek(16);
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        const int hi = h.maxcode[l], lo = h.mincode[l];
        if (hi >= 0 && c <= hi && c >= lo) { br.skip(l); return h.vals[(h.valptr[l] + c - lo) & 255]; }
    }
    br.skip(16);
    return 0;
}
__device__ inline int jpeg_extend(int v, int s) { return s == 0 ? 0 : (v < (1 << (s - 1)) ? v - (1 << s) + 1 : v); }

__global__ __launch_bounds__(JPEG_HUFF_LANES) void jpeg_huffman_kernel(JpegGeom G, const uint8_t* __restrict__ scan, const uint32_t* __restrict__ seg,
                                                                      const uint32_t* __restrict__ tables, int16_t* __restrict__ coef, int32_t* __restrict__ status)
{
    __shared__ uint32_t lds[JPEG_HUFF_LDS_BYTES / 4];
    for (int i = threadIdx.x; i < JPEG_HUFF_LDS_BYTES / 4; i += JPEG_HUFF_LANES) lds[i] = tables[i];
    // the blocks of this workgroup's intervals start as zeros: only non-zero coefficients are stored below
    const long long mcu_lo = (long long)blockIdx.x * JPEG_HUFF_INTERVALS * G.ri;
    const long long mcu_hi = min(mcu_lo + (long long)JPEG_HUFF_INTERVALS * G.ri, (long long)G.nmcu);
    // (at most 2^22 MCUs of at most 48 blocks: the count fits 32 bits)
    const unsigned items = mcu_hi > mcu_lo ? (unsigned)(mcu_hi - mcu_lo) * (unsigned)G.bpm * 8u : 0u;
    for (unsigned it = threadIdx.x; it < items; it += JPEG_HUFF_LANES) {
        const unsigned b = it >> 3;
        const unsigned m = b / (unsigned)G.bpm;
        const unsigned blk = jpeg_block_of(G, (int)(mcu_lo + m), (int)(b - m * (unsigned)G.bpm));
        reinterpret_cast<uint4*>(coef)[(size_t)blk * 8 + (size_t)(it & 7)] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    // with one interval per workgroup the interval, and with it every value below, is uniform over the wave: the compiler keeps the
    // bit reader's state in scalar registers and its arithmetic on the scalar unit
    const int interval = JPEG_HUFF_INTERVALS == 1 ? (int)blockIdx.x : (int)(blockIdx.x * JPEG_HUFF_INTERVALS + threadIdx.x / JPEG_HUFF_STRIDE);
    if (threadIdx.x % JPEG_HUFF_STRIDE != 0 || interval >= G.n_int) return;
    const JpegHuffDev* T = reinterpret_cast<const JpegHuffDev*>(lds);
    const uint8_t* zz = reinterpret_cast<const uint8_t*>(lds) + JPEG_HUFF_TABLES * JPEG_HUFF_TABLE_BYTES;
    JpegBits br; br.s = reinterpret_cast<const uint4*>(scan); br.p = seg[2 * interval]; br.e = seg[2 * interval + 1]; br.acc = 0; br.n = 0;
    br.wi = 0xFFFFFFFFu; br.lo = br.hi = 0;
    int pred[3] = { 0, 0, 0 };
    const int m0 = interval * G.ri, m1 = min(m0 + G.ri, G.nmcu);
    for (int mcu = m0; mcu < m1; ++mcu) {
        const int my = mcu / G.mcux, mx = mcu - my * G.mcux;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= G.ncomp) break;
            const JpegHuffDev& hdc = T[G.c[c].td];
            const JpegHuffDev& hac = T[4 + G.c[c].ta];
            for (int by = 0; by < G.c[c].v; ++by)
                for (int bx = 0; bx < G.c[c].h; ++bx) {
                    int16_t* cb = coef + ((size_t)G.c[c].blk0 + (size_t)(my * G.c[c].v + by) * G.c[c].bw + (size_t)(mx * G.c[c].h + bx)) * 64;
                    int s = jpeg_decode_symbol(br, hdc);
                    if (s > 11) { atomicOr(status, JPEG_BAD_DC_CATEGORY); return; }
                    pred[c] += jpeg_extend(br.get(s), s);
                    if (pred[c] < -32768 || pred[c] > 32767) { atomicOr(status, JPEG_BAD_PREDICTOR); return; }
                    if (pred[c]) cb[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = jpeg_decode_symbol(br, hac);
                        const int r = rs >> 4; s = rs & 15;
                        if (s == 0) { if (r == 15) { k += 16; continue; } break; }
                        k += r;
                        if (k > 63) { atomicOr(status, JPEG_BAD_RUN); return; }
                        if (s > 10) { atomicOr(status, JPEG_BAD_AC_CATEGORY); return; }
                        cb[zz[k]] = (int16_t)jpeg_extend(br.get(s), s);
                        ++k;
                    }
                }
        }
    }
}

// Eight lanes per block: lane c runs the column pass of column c into the LDS workspace, then lane r the row pass of row r and
// stores its eight samples as one 8-byte word.  The products and sums are decode_jpeg's: an int product, then idct_1d.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegGeom G, const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, uint8_t* __restrict__ planes,
                                                        unsigned nblocks)
{
    __shared__ int ws[JPEG_IDCT_BLOCKS * JPEG_WS_BLOCK];
    const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const unsigned b = blockIdx.x * JPEG_IDCT_BLOCKS + slot;
    const bool on = b < nblocks;
    int* w = ws + slot * JPEG_WS_BLOCK;
    int c = 0;
    long long o[8];
    if (on) {
        if (G.ncomp > 1 && b >= G.c[1].blk0) c = 1;
        if (G.ncomp > 2 && b >= G.c[2].blk0) c = 2;
        const int16_t* in = coef + (size_t)b * 64 + lane;
        const uint16_t* q = qt + G.c[c].tq * 64 + lane;
        sfm::jpeg::idct_1d((int)in[0] * (int)q[0], (int)in[8] * (int)q[8], (int)in[16] * (int)q[16], (int)in[24] * (int)q[24],
                           (int)in[32] * (int)q[32], (int)in[40] * (int)q[40], (int)in[48] * (int)q[48], (int)in[56] * (int)q[56], o);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[JPEG_WS_ROW * r + lane] = sfm::jpeg::descale(o[r], 11);
    }
    __syncthreads();
    if (!on) return;
    const int* row = w + JPEG_WS_ROW * lane;
    sfm::jpeg::idct_1d(row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7], o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)sfm::jpeg::clamp_sample(sfm::jpeg::descale(o[k], 18)) << (8 * k);
        hi |= (uint32_t)sfm::jpeg::clamp_sample(sfm::jpeg::descale(o[4 + k], 18)) << (8 * k);
    }
    const unsigned rel = b - G.c[c].blk0;
    const unsigned brow = rel / (unsigned)G.c[c].bw, bcol = rel - brow * (unsigned)G.c[c].bw;
    uint8_t* dst = planes + G.c[c].plane0 + ((size_t)brow * 8 + lane) * (size_t)G.c[c].pw + (size_t)bcol * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// sample (x, y) of the full-resolution plane upsample() would build from component C: its branches in closed form
__device__ inline int jpeg_sample(const JpegGeom& G, const JpegComp& C, const uint8_t* __restrict__ planes, int x, int y)
{
    const uint8_t* src = planes + C.plane0;
    const int hr = G.hmax / C.h, vr = G.vmax / C.v, cs = C.pw, cw = C.w, ch = C.hgt;
    if (hr == 1 && vr == 1) return src[(size_t)y * cs + x];
    if (hr == 2 && vr == 1 && cw > 2) {                  // h2v1 fancy
        const uint8_t* in = src + (size_t)y * cs;
        const int k = x >> 1;
        if (x & 1) return k == cw - 1 ? in[k] : (in[k] * 3 + in[k + 1] + 2) >> 2;
        return k == 0 ? in[0] : (in[k] * 3 + in[k - 1] + 1) >> 2;
    }
    if (hr == 2 && vr == 2 && cw > 2) {                  // h2v2 fancy
        const int iy = y >> 1;
        int ny = (y & 1) ? iy + 1 : iy - 1;
        if (ny < 0) ny = 0;
        if (ny > ch - 1) ny = ch - 1;
        const uint8_t* in0 = src + (size_t)iy * cs; const uint8_t* in1 = src + (size_t)ny * cs;
        const int k = x >> 1;
        const int thiscol = in0[k] * 3 + in1[k];
        if (x & 1) return k == cw - 1 ? (thiscol * 4 + 7) >> 4 : (thiscol * 3 + (in0[k + 1] * 3 + in1[k + 1]) + 7) >> 4;
        return k == 0 ? (thiscol * 4 + 8) >> 4 : (thiscol * 3 + (in0[k - 1] * 3 + in1[k - 1]) + 8) >> 4;
    }
    return src[(size_t)(y / vr) * cs + x / hr];          // replication
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(JpegGeom G, const uint8_t* __restrict__ planes, const int* __restrict__ ycc, uint8_t* __restrict__ img, size_t ld)
{
    __shared__ int tab[4 * 256];                // cr_r, cb_b, cr_g, cb_g
    const int t = threadIdx.y * 64 + threadIdx.x;
    if (G.ncomp == 3) {
        for (int i = t; i < 4 * 256; i += 256) tab[i] = ycc[i];
        __syncthreads();
    }
    const int y = blockIdx.y * 4 + threadIdx.y;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * JPEG_RUN;
    if (y >= G.H || x0 >= G.W) return;
    const int x1 = min(x0 + JPEG_RUN, G.W);
    uint8_t* out = img + (size_t)y * ld;
    if (G.ncomp == 1) {
        const uint8_t* src = planes + G.c[0].plane0 + (size_t)y * G.c[0].pw;
        for (int x = x0; x < x1; ++x) out[x] = src[x];
        return;
    }
    for (int x = x0; x < x1; ++x) {
        const int Y = jpeg_sample(G, G.c[0], planes, x, y), cb = jpeg_sample(G, G.c[1], planes, x, y), cr = jpeg_sample(G, G.c[2], planes, x, y);
        const int r = Y + tab[cr], g = Y + ((tab[768 + cb] + tab[512 + cr]) >> 16), b = Y + tab[256 + cb];
        out[3 * (size_t)x + 0] = (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
        out[3 * (size_t)x + 1] = (uint8_t)(g < 0 ? 0 : g > 255 ? 255 : g);
        out[3 * (size_t)x + 2] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
    }
}

// ---- host side ----

struct JpegPlan {
    Frame fr;
    JpegGeom G;
    unsigned nblocks = 0;
    size_t plane_bytes = 0;
    bool device_entropy = false;
    std::vector<uint32_t> seg;          // device entropy: [start, end) of every interval, relative to the scan's start
    // host entropy: the coefficients.  Pageable on purpose: sfm_upload has consumed them (through the pinned staging ring) when it
    // returns, which an enqueue-only call needs; the context's one pinned block could still be the source of the previous call's copy
    std::vector<int16_t> coef;
    int channels() const { return G.ncomp == 1 ? 1 : 3; }
};

// Automatic choice of the entropy stage: the device from this many restart intervals on.  Measured (profiles/r18_time_jpeg.log, the
// sweep of experiments/time_jpeg.py): both stages take time in proportion to the number of blocks, the host's one thread about 64 ns
// per block with the upload of its coefficients, a device lane about 2.7 us per block, so the break-even is a number of intervals and
// not a size: at 3648 x 2736 the device loses at 22 intervals (28.9 against 15.5 ms), ties at 43 (14.8 / 15.3) and wins at 86 (7.6 /
// 15.3); at 1024 x 768 it wins at 48 (1.18 against 1.37 ms).  (Before that measurement the value was a guessed 64.)
constexpr int JPEG_DEVICE_MIN_INTERVALS = 48;

// [start, end) of the first `want` segments of the scan d[0 .. len); false: fewer restart markers than that needs
bool jpeg_segments(const uint8_t* d, size_t len, long long want, std::vector<uint32_t>& seg)
{
    seg.clear(); seg.reserve((size_t)want * 2);
    size_t start = 0, at = 0;
    for (long long k = 0; k < want; ++k) {
        size_t end = len;                                   // the next FF D0..D7 at or after `at`
        bool found = false;
        while (at + 1 < len) {
            const uint8_t* q = (const uint8_t*)memchr(d + at, 0xFF, len - 1 - at);
            if (!q) break;
            at = (size_t)(q - d);
            if (d[at + 1] >= 0xD0 && d[at + 1] <= 0xD7) { end = at; found = true; break; }
            ++at;
        }
        if (!found && k + 1 < want) return false;
        seg.push_back((uint32_t)start); seg.push_back((uint32_t)end);
        start = at = end + 2;
    }
    return true;
}

// everything that can be refused is refused here, before anything is enqueued or written
int jpeg_plan(sfmhip_ctx* ctx, const uint8_t* bytes, size_t n, int entropy, JpegPlan& P)
{
    auto refuse = [&](const char* why) { if (ctx) ctx->last_error = std::string("jpeg: ") + why; return SFMHIP_E_ARG; };
    if (n >= ((size_t)1 << 31)) return refuse("a file of 2 GiB or more");
    Frame& fr = P.fr;
    if (!sfm::jpeg::parse_headers(bytes, n, fr)) return refuse("not a baseline JPEG this decoder supports (progressive, arithmetic, 12-bit, CMYK / RGB-coded), or damaged headers");
    JpegGeom& G = P.G;
    memset(&G, 0, sizeof G);
    G.W = fr.W; G.H = fr.H; G.ncomp = (int)fr.comp.size(); G.hmax = fr.hmax; G.vmax = fr.vmax; G.mcux = fr.mcux; G.mcuy = fr.mcuy;
    G.nmcu = (int)fr.mcus(); G.ri = fr.restart ? fr.restart : G.nmcu; G.n_int = (int)fr.intervals();
    unsigned blk = 0; size_t plane = 0;
    for (int c = 0; c < G.ncomp; ++c) {
        const sfm::jpeg::Component& s = fr.comp[(size_t)c];
        JpegComp& d = G.c[c];
        d.h = s.h; d.v = s.v; d.tq = s.tq; d.td = s.td; d.ta = s.ta; d.w = s.w; d.hgt = s.hgt; d.pw = s.pw; d.ph = s.ph; d.bw = s.pw / 8;
        d.blk0 = blk; d.plane0 = (unsigned)plane;
        blk += (unsigned)(s.pw / 8) * (unsigned)(s.ph / 8); plane += align256((size_t)s.pw * s.ph);
        G.bpm += s.h * s.v;
    }
    P.nblocks = blk; P.plane_bytes = plane;
    P.device_entropy = entropy == 2 || (entropy == 0 && fr.restart > 0 && G.n_int >= JPEG_DEVICE_MIN_INTERVALS);
    if (P.device_entropy) {
        if (!jpeg_segments(bytes + fr.scan, n - fr.scan, G.n_int, P.seg)) return refuse("fewer restart markers than restart intervals");
    } else {
        P.coef.assign((size_t)P.nblocks * 64, 0);
        const bool ok = sfm::jpeg::decode_scan(bytes, n, fr, [&](int ci, int brow, int bcol, const int* qc) {
            int16_t* cb = P.coef.data() + ((size_t)G.c[ci].blk0 + (size_t)brow * G.c[ci].bw + bcol) * 64;
            for (int z = 0; z < 64; ++z) cb[z] = (int16_t)qc[z];
        });
        if (!ok) return refuse("corrupt entropy-coded data");
    }
    return SFMHIP_OK;
}

// the chain on the context's stream; the temporaries go back to the cache when `hold` does (stream-ordered reuse)
int jpeg_enqueue(sfmhip_ctx* ctx, SfmPoolHold& hold, const JpegPlan& P, const uint8_t* bytes, size_t n, uint8_t* d_img, size_t ld, int32_t* d_status)
{
    const JpegGeom& G = P.G; const Frame& fr = P.fr;
    const size_t scan_len = n - fr.scan;
    std::vector<uint8_t> blob(JPEG_OFF_SEG + P.seg.size() * 4, 0);
    for (int t = 0; t < JPEG_HUFF_TABLES; ++t) {
        const Huff& h = t < 4 ? fr.hdc[t] : fr.hac[t - 4];
        if (!h.present) continue;
        JpegHuffDev* d = reinterpret_cast<JpegHuffDev*>(blob.data() + (size_t)t * JPEG_HUFF_TABLE_BYTES);
        memcpy(d->look, h.look, sizeof d->look); memcpy(d->mincode, h.mincode, sizeof d->mincode);
        memcpy(d->maxcode, h.maxcode, sizeof d->maxcode); memcpy(d->valptr, h.valptr, sizeof d->valptr); memcpy(d->vals, h.vals, sizeof d->vals);
    }
    memcpy(blob.data() + JPEG_HUFF_TABLES * JPEG_HUFF_TABLE_BYTES, sfm::jpeg::kZigzag, 64);
    for (int t = 0; t < 4; ++t) if (fr.qt_ok[t]) memcpy(blob.data() + JPEG_OFF_QT + (size_t)t * 128, fr.qt[t], 128);
    {
        int cr_r[256], cb_b[256]; long cr_g[256], cb_g[256];
        sfm::jpeg::ycc_tables(cr_r, cb_b, cr_g, cb_g);
        int* y = reinterpret_cast<int*>(blob.data() + JPEG_OFF_YCC);
        for (int k = 0; k < 256; ++k) { y[k] = cr_r[k]; y[256 + k] = cb_b[k]; y[512 + k] = (int)cr_g[k]; y[768 + k] = (int)cb_g[k]; }
    }
    if (!P.seg.empty()) memcpy(blob.data() + JPEG_OFF_SEG, P.seg.data(), P.seg.size() * 4);

    SfmCarve carve;
    const size_t o_blob = carve(blob.size()), o_scan = carve(P.device_entropy ? (scan_len + 15) / 16 * 16 : 0), o_coef = carve((size_t)P.nblocks * 128), o_planes = carve(P.plane_bytes);
    char* base = nullptr;
    int rc = hold.get(carve.bytes, (void**)&base);
    if (rc != SFMHIP_OK) return rc;
    SFM_HIP_TRY(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t), ctx->stream));
    rc = sfm_upload(ctx, base + o_blob, blob.data(), blob.size());
    if (rc != SFMHIP_OK) return rc;
    int16_t* d_coef = reinterpret_cast<int16_t*>(base + o_coef);
    if (P.device_entropy) {
        rc = sfm_upload(ctx, base + o_scan, bytes + fr.scan, scan_len);
        if (rc != SFMHIP_OK) return rc;
        jpeg_huffman_kernel<<<ceil_div(G.n_int, JPEG_HUFF_INTERVALS), JPEG_HUFF_LANES, 0, ctx->stream>>>(
            G, reinterpret_cast<const uint8_t*>(base + o_scan), reinterpret_cast<const uint32_t*>(base + o_blob + JPEG_OFF_SEG),
            reinterpret_cast<const uint32_t*>(base + o_blob), d_coef, d_status);
    } else {
        rc = sfm_upload(ctx, d_coef, P.coef.data(), P.coef.size() * sizeof(int16_t));
        if (rc != SFMHIP_OK) return rc;
    }
    uint8_t* d_planes = reinterpret_cast<uint8_t*>(base + o_planes);
    jpeg_idct_kernel<<<(P.nblocks + JPEG_IDCT_BLOCKS - 1) / JPEG_IDCT_BLOCKS, 256, 0, ctx->stream>>>(
        G, d_coef, reinterpret_cast<const uint16_t*>(base + o_blob + JPEG_OFF_QT), d_planes, P.nblocks);
    jpeg_colour_kernel<<<dim3((unsigned)ceil_div(G.W, 64 * JPEG_RUN), (unsigned)ceil_div(G.H, 4)), dim3(64, 4), 0, ctx->stream>>>(
        G, d_planes, reinterpret_cast<const int*>(base + o_blob + JPEG_OFF_YCC), d_img, ld);
    SFM_HIP_TRY(ctx, hipGetLastError());
    return SFMHIP_OK;
}

}  // namespace

extern "C" {

int sfmhip_jpeg_info(const uint8_t* bytes, size_t n, int* rows, int* cols, int* channels, int* restart_interval, int* n_intervals)
{
    if (!bytes || !rows || !cols || !channels || !restart_interval || !n_intervals) return SFMHIP_E_ARG;
    Frame fr;
    if (n >= ((size_t)1 << 31) || !sfm::jpeg::parse_headers(bytes, n, fr)) return SFMHIP_E_ARG;
    *rows = fr.H; *cols = fr.W; *channels = fr.comp.size() == 1 ? 1 : 3; *restart_interval = fr.restart; *n_intervals = (int)fr.intervals();
    return SFMHIP_OK;
}

int sfmhip_jpeg_decode_dev(sfmhip_ctx* ctx, const uint8_t* bytes, size_t n, int entropy, uint8_t* d_img, size_t ld, int32_t* d_status)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_jpeg_decode_dev");
    SFM_ARG_CHECK(ctx, ctx && bytes && d_img && d_status && entropy >= 0 && entropy <= 2);
    JpegPlan P;
    int rc = jpeg_plan(ctx, bytes, n, entropy, P);
    if (rc != SFMHIP_OK) return rc;
    SFM_ARG_CHECK(ctx, ld >= (size_t)P.G.W * P.channels());
    SfmPoolHold hold(ctx);
    return jpeg_enqueue(ctx, hold, P, bytes, n, d_img, ld, d_status);
}

int sfmhip_jpeg_decode(sfmhip_ctx* ctx, const uint8_t* bytes, size_t n, int entropy, uint8_t* img, size_t ld)
{
    SFM_DEVICE_GUARD(ctx);
    SFM_RANGE("sfmhip_jpeg_decode");
    SFM_ARG_CHECK(ctx, ctx && bytes && img && entropy >= 0 && entropy <= 2);
    JpegPlan P;
    int rc = jpeg_plan(ctx, bytes, n, entropy, P);
    if (rc != SFMHIP_OK) return rc;
    const size_t row = (size_t)P.G.W * P.channels();
    SFM_ARG_CHECK(ctx, ld >= row);
    SfmPoolHold hold(ctx);
    uint8_t* d_img = nullptr; int32_t* d_status = nullptr;
    rc = hold.get(row * P.G.H, (void**)&d_img);
    if (rc == SFMHIP_OK) rc = hold.get(&d_status, 1);
    if (rc == SFMHIP_OK) rc = jpeg_enqueue(ctx, hold, P, bytes, n, d_img, row, d_status);
    if (rc != SFMHIP_OK) return sfm_drain(ctx, rc);
    int32_t status = 0;
    hipError_t e = hipMemcpyAsync(&status, d_status, sizeof status, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && status == 0) e = hipMemcpy2DAsync(img, ld, d_img, row, row, (size_t)P.G.H, hipMemcpyDeviceToHost, ctx->stream);
    rc = sfm_finish(ctx, e);
    if (rc != SFMHIP_OK) return rc;
    if (status != 0) { ctx->last_error = "jpeg: corrupt entropy-coded data (status " + std::to_string(status) + ")"; return SFMHIP_E_ARG; }
    return SFMHIP_OK;
}

}  // extern "C"
