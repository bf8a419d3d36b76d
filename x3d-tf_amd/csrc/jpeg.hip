// x3d_jpeg_parse / x3d_jpeg_decode: baseline JPEG decoding of TFRecord frames on the GPU.
//
// Scope (ITU-T T.81): SOF0 / SOF1, 8-bit samples, Huffman coding, one interleaved scan holding every component,
// 1 component (grey) or 3 (YCbCr: luma 1x1, 2x1 or 2x2, chroma 1x1), optional DRI / RSTn, any extents.  Everything
// else is reported per image as X3D_JPEG_UNSUPPORTED / X3D_JPEG_MALFORMED and left to the caller's host decoder.
//
// The result must be bit-identical to the host decoder's defaults (libjpeg(-turbo) as Pillow drives it):
//   - the ISLOW integer IDCT: the Loeffler-Ligtenberg-Moschytz factorisation, 13-bit constants, 2 extra bits between
//     the passes, output + 128 limited to [0, 255];
//   - "fancy" chroma upsampling: triangle filter, 3/4 nearer + 1/4 further sample, horizontally (h2v1) or in both
//     directions (h2v2), the rounding biases alternating between output columns, samples beyond the component's
//     downsampled extent replaced by the edge sample; components two samples wide or less are replicated instead;
//   - the 16-bit fixed-point YCbCr -> RGB conversion with its rounded per-value terms, limited to [0, 255];
//   - grey replicated to R, G, B.
//
// Three launches per batch, every loop bounded by its image's byte range or block count:
//   1. entropy: one wave per image.  The wave builds the image's Huffman lookup tables in LDS from the raw DHT bytes,
//      then lane 0 decodes the (inherently sequential) scan: byte stuffing removed while reading, DC prediction,
//      restart intervals.  Quantised coefficients go to an int16 scratch in natural order.  A stream that runs out
//      early, an invalid code, a wrong restart marker or a marker behind the last MCU sets the image's status word
//      and stops that image.
//   2. idct: one thread per 8x8 block: dequantise + ISLOW IDCT into uint8 component planes.  A block outside the
//      range in which the host decoders agree (kCoefLimit ...) sets the status word too.
//   3. color: one thread per output pixel: upsample + convert, straight into the caller's [H][W][3] slot.
#include "common.h"

#include <string.h>

namespace {

constexpr int kLook = 9;                 // Huffman lookahead bits
constexpr int kTables = 8;               // DC 0-3, AC 0-3

constexpr unsigned char kZigzag[64] = {  // zig-zag position -> natural (row-major) position, T.81 figure A.6
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------
// host: header parse
// ------------------------------------------------------------------------------------------------
static inline int rd16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// checks one DHT table the way a baseline decoder must before building it: at most 256 symbols, canonical codes that
// fit their lengths, DC categories <= 15.  Returns false for a table the host decoder would refuse.
static bool huff_table_ok(const unsigned char* counts, const unsigned char* vals, bool dc) {
  int total = 0, last = 0;
  for (int l = 1; l <= 16; l++) {
    total += counts[l - 1];
    if (counts[l - 1]) last = l;
  }
  if (total > 256) return false;
  long code = 0;
  for (int l = 1; l <= last; l++) {   // codes of length l are code .. code + count - 1; the all-ones code stays unused
    code += counts[l - 1];
    if (code >= (1l << l)) return false;
    code <<= 1;
  }
  if (dc)
    for (int i = 0; i < total; i++)
      if (vals[i] > 15) return false;
  return true;
}

static void parse_one(const unsigned char* p, int len, x3d_jpeg_image* d) {
  const int H_MAL = X3D_JPEG_MALFORMED, H_UNS = X3D_JPEG_UNSUPPORTED;
  d->status = H_MAL;
  d->height = d->width = d->ncomp = 0;
  d->restart_interval = 0;
  d->ecs_off = d->ecs_end = 0;
  for (int i = 0; i < kTables; i++) d->huff_off[i] = -1;
  int qoff[4] = {-1, -1, -1, -1}, qprec[4] = {0, 0, 0, 0};
  int comp_id[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  int unsupported = 0;
  if (!p || len < 4 || p[0] != 0xFF || p[1] != 0xD8) return;
  int pos = 2;
  while (true) {
    // next marker: any number of 0xFF fill bytes, then the code
    if (pos >= len || p[pos] != 0xFF) return;
    while (pos < len && p[pos] == 0xFF) pos++;
    if (pos >= len) return;
    const int m = p[pos++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
    if (m == 0xD9) return;                                                // EOI before SOS
    if (pos + 2 > len) return;
    const int seg = rd16(p + pos);
    if (seg < 2 || pos + seg > len) return;
    const unsigned char* s = p + pos + 2;
    const int n = seg - 2;
    if (m == 0xC0 || m == 0xC1) {                                         // SOF0 / SOF1
      if (have_sof || n < 6) return;
      have_sof = true;
      const int prec = s[0];
      d->height = rd16(s + 1);
      d->width = rd16(s + 3);
      d->ncomp = s[5];
      if (d->ncomp < 1 || n != 6 + 3 * d->ncomp) return;
      if (d->width == 0) return;
      if (prec != 8) unsupported = 1;
      if (d->height == 0) unsupported = 1;                                // DNL
      if (d->ncomp != 1 && d->ncomp != 3) unsupported = 1;
      for (int c = 0; c < d->ncomp && c < 3; c++) {
        comp_id[c] = s[6 + 3 * c];
        d->hs[c] = s[7 + 3 * c] >> 4;
        d->vs[c] = s[7 + 3 * c] & 15;
        comp_q[c] = s[8 + 3 * c];
        if (d->hs[c] < 1 || d->hs[c] > 4 || d->vs[c] < 1 || d->vs[c] > 4 || comp_q[c] > 3) return;
      }
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (have_sof) return;
      have_sof = true;
      unsupported = 1;                                                    // progressive, lossless, arithmetic
      if (n >= 6) { d->height = rd16(s + 1); d->width = rd16(s + 3); d->ncomp = s[5]; }
      d->status = H_UNS;
      return;
    } else if (m == 0xCC) {                                               // DAC: arithmetic conditioning
      unsupported = 1;
    } else if (m == 0xDB) {                                               // DQT
      int q = 0;
      while (q < n) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (tq > 3 || pq > 1) return;
        const int need = 1 + 64 * (pq ? 2 : 1);
        if (q + need > n) return;
        qoff[tq] = (int)(s + q + 1 - p);
        qprec[tq] = pq;
        q += need;
      }
    } else if (m == 0xC4) {                                               // DHT
      int q = 0;
      while (q < n) {
        if (q + 17 > n) return;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return;
        int total = 0;
        for (int l = 0; l < 16; l++) total += s[q + 1 + l];
        if (total > 256 || q + 17 + total > n) return;
        if (!huff_table_ok(s + q + 1, s + q + 17, tc == 0)) return;
        d->huff_off[tc * 4 + th] = (int)(s + q + 1 - p);
        q += 17 + total;
      }
    } else if (m == 0xDD) {                                               // DRI
      if (n != 2) return;
      d->restart_interval = rd16(s);
    } else if (m == 0xE0) {                                               // APP0: JFIF
      if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {                                               // APP14: Adobe
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {                                               // SOS
      if (!have_sof || n < 1) return;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return;
      if (unsupported) { d->status = H_UNS; return; }
      if (ns != d->ncomp) { d->status = H_UNS; return; }                  // multi-scan sequential
      for (int i = 0; i < ns; i++) {
        const int cid = s[1 + 2 * i];
        int c = -1;
        for (int k = 0; k < d->ncomp; k++)
          if (comp_id[k] == cid) c = k;
        if (c < 0) return;
        const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
        if (td > 3 || ta > 3) return;
        d->dc_tbl[c] = td;
        d->ac_tbl[c] = ta;
      }
      const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
      if (ss != 0 || se != 63 || ahal != 0) return;
      for (int c = 0; c < d->ncomp; c++) {
        if (d->huff_off[d->dc_tbl[c]] < 0 || d->huff_off[4 + d->ac_tbl[c]] < 0) return;
        if (qoff[comp_q[c]] < 0) return;
      }
      // colour space as a baseline decoder infers it: JFIF -> YCbCr; Adobe transform 0 -> RGB (or CMYK);
      // neither marker and component ids 'R', 'G', 'B' -> RGB
      if (d->ncomp == 3) {
        if (!jfif && adobe && adobe_transform == 0) { d->status = H_UNS; return; }
        if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') { d->status = H_UNS; return; }
        const int hy = d->hs[0], vy = d->vs[0];
        const bool chroma11 = d->hs[1] == 1 && d->vs[1] == 1 && d->hs[2] == 1 && d->vs[2] == 1;
        if (!chroma11 || !((hy == 1 && vy == 1) || (hy == 2 && vy == 1) || (hy == 2 && vy == 2))) {
          d->status = H_UNS;
          return;
        }
      }
      for (int c = 0; c < d->ncomp; c++) {
        const unsigned char* qt = p + qoff[comp_q[c]];
        for (int k = 0; k < 64; k++) {
          const int v = qprec[comp_q[c]] ? rd16(qt + 2 * k) : qt[k];
          if (v > 255) { d->status = H_UNS; return; }                    // 16-bit products: not the 8-bit path
          d->qt[c][kZigzag[k]] = (unsigned short)v;
        }
      }
      d->ecs_off = pos + seg;
      // the entropy-coded segment runs to the last EOI (markers inside it are RSTn; the device checks them)
      int end = len;
      for (int i = len - 2; i >= d->ecs_off; i--)
        if (p[i] == 0xFF && p[i + 1] == 0xD9) { end = i; break; }
      d->ecs_end = end;
      if (d->ncomp == 1) {                                                // non-interleaved: one block per MCU
        d->hs[0] = d->vs[0] = 1;
        d->mcux = (d->width + 7) / 8;
        d->mcuy = (d->height + 7) / 8;
        d->bw[0] = d->mcux;
        d->bh[0] = d->mcuy;
      } else {
        const int hm = d->hs[0], vm = d->vs[0];
        d->mcux = (d->width + 8 * hm - 1) / (8 * hm);
        d->mcuy = (d->height + 8 * vm - 1) / (8 * vm);
        for (int c = 0; c < 3; c++) { d->bw[c] = d->mcux * d->hs[c]; d->bh[c] = d->mcuy * d->vs[c]; }
      }
      d->status = X3D_JPEG_OK;
      return;
    }
    pos += seg;
  }
}

static long long blocks_of(const x3d_jpeg_image* d) {
  long long b = 0;
  for (int c = 0; c < d->ncomp; c++) b += (long long)d->bw[c] * d->bh[c];
  return b;
}

static inline long long align256(long long x) { return (x + 255) & ~255ll; }

}  // namespace

extern "C" int x3d_jpeg_parse(const unsigned char* const* data, const int* lengths, int n, x3d_jpeg_image* imgs,
                              long long* scratch_bytes) {
  X3D_REQUIRE(n >= 0 && (n == 0 || (data && lengths && imgs)), "jpeg_parse: null pointer");
  long long coef = 0;
  for (int i = 0; i < n; i++) {
    x3d_jpeg_image* d = imgs + i;
    parse_one(data[i], lengths[i], d);
    d->coef_off = d->plane_off = 0;
    if (d->status == X3D_JPEG_OK) {
      d->coef_off = coef;
      coef = align256(coef + blocks_of(d) * 128);
    }
  }
  long long planes = coef;
  for (int i = 0; i < n; i++) {
    x3d_jpeg_image* d = imgs + i;
    if (d->status == X3D_JPEG_OK) {
      d->plane_off = planes;
      planes = align256(planes + blocks_of(d) * 64);
    }
  }
  if (scratch_bytes) *scratch_bytes = planes;
  return X3D_OK;
}

// ------------------------------------------------------------------------------------------------
// device: entropy decode
// ------------------------------------------------------------------------------------------------
namespace {

struct HuffLds {
  unsigned short look[kTables][1 << kLook];   // (length << 8) | symbol for codes up to kLook bits; 0: longer code
  int maxcode[kTables][18];                   // largest code of each length (-1: none), [17] sentinel
  int valoff[kTables][17];                    // symbol index = valoff[l] + code
  unsigned char vals[kTables][256];
};

struct BitReader {
  const unsigned char* p;
  const unsigned char* end;
  unsigned long long acc;   // next bit at bit 63
  int n;                    // bits in acc
  int marker;               // reached a marker (or the segment end): zeros are shifted in from here on
  long long real, used;     // bits loaded from the stream / consumed since the last restart

  __host__ __device__ inline void fill() {
    while (n <= 56) {
      unsigned c = 0;
      if (!marker) {
        if (p < end) {
          c = p[0];
          if (c == 0xFF) {
            if (p + 1 < end && p[1] == 0x00) { p += 2; real += 8; }
            else { marker = 1; c = 0; }                                   // p stays on the marker
          } else { p++; real += 8; }
        } else {
          marker = 1;
        }
      }
      acc |= (unsigned long long)c << (56 - n);
      n += 8;
    }
  }
  __host__ __device__ inline unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }
  __host__ __device__ inline void skip(int k) { acc <<= k; n -= k; used += k; }
};

// decodes one Huffman symbol; -1 on an invalid code.  acc holds >= 57 bits (fill() before).
__host__ __device__ inline int huff_decode(BitReader& br, const HuffLds& t, int tb) {
  const unsigned e = t.look[tb][br.peek(kLook)];
  if (e >> 8) {
    br.skip(e >> 8);
    return e & 255;
  }
  for (int l = kLook + 1; l <= 16; l++) {
    const int code = (int)br.peek(l);
    if (code <= t.maxcode[tb][l]) {
      br.skip(l);
      return t.vals[tb][(t.valoff[tb][l] + code) & 255];
    }
  }
  return -1;
}

__host__ __device__ inline int extend(unsigned r, int s) { return r < (1u << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r; }

// canonical code limits of table `tb` (the host validated counts and lengths)
__host__ __device__ inline void huff_limits(const unsigned char* base, const x3d_jpeg_image& d, HuffLds& t, int tb) {
  const int off = d.huff_off[tb];
  int code = 0, p = 0;
  for (int l = 1; l <= 16; l++) {
    const int cnt = off >= 0 ? base[off + l - 1] : 0;
    if (cnt) {
      t.valoff[tb][l] = p - code;
      code += cnt;
      p += cnt;
      t.maxcode[tb][l] = code - 1;
    } else {
      t.valoff[tb][l] = 0;
      t.maxcode[tb][l] = -1;
    }
    code <<= 1;
  }
  t.maxcode[tb][17] = 0x7fffffff;
  for (int i = 0; i < 256; i++) t.vals[tb][i] = (off >= 0 && i < p) ? base[off + 16 + i] : 0;
}

// lookup entry e = (table << kLook) | next kLook bits
__host__ __device__ inline void huff_look(HuffLds& t, int e) {
  const int tb = e >> kLook, v = e & ((1 << kLook) - 1);
  unsigned short r = 0;
  for (int l = 1; l <= kLook; l++) {
    const int code = v >> (kLook - l);
    if (code <= t.maxcode[tb][l]) {
      r = (unsigned short)((l << 8) | t.vals[tb][(t.valoff[tb][l] + code) & 255]);
      break;
    }
  }
  t.look[tb][v] = r;
}

// the scan of one image -> quantised coefficients (natural order) in `coef`, which the caller zeroed; X3D_JPEG_OK or
// X3D_JPEG_CORRUPT
__host__ __device__ inline int entropy_decode(const unsigned char* base, const x3d_jpeg_image& d, const HuffLds& t,
                                              short* coef) {
  long long comp_base[3] = {0, 0, 0};
  for (int c = 1; c < d.ncomp; c++) comp_base[c] = comp_base[c - 1] + (long long)d.bw[c - 1] * d.bh[c - 1] * 64;
  BitReader br;
  br.p = base + d.ecs_off;
  br.end = base + d.ecs_end;
  br.acc = 0; br.n = 0; br.marker = 0; br.real = 0; br.used = 0;
  int pred[3] = {0, 0, 0};
  int rst = 0;
  const int ri = d.restart_interval;
  const long long mcus = (long long)d.mcux * d.mcuy;
  for (long long m = 0; m < mcus; m++) {
    if (ri && m > 0 && m % ri == 0) {
      // restart: the interval's data must be used up to the byte padding, then RSTn follows
      if (br.real - br.used >= 8) return X3D_JPEG_CORRUPT;
      const unsigned char* q = br.p;
      while (q + 1 < br.end && q[0] == 0xFF && q[1] == 0xFF) q++;
      if (!(q + 1 < br.end && q[0] == 0xFF && q[1] == 0xD0 + rst)) return X3D_JPEG_CORRUPT;
      br.p = q + 2;
      br.acc = 0; br.n = 0; br.marker = 0; br.real = 0; br.used = 0;
      pred[0] = pred[1] = pred[2] = 0;
      rst = (rst + 1) & 7;
    }
    const int mx = (int)(m % d.mcux), my = (int)(m / d.mcux);
    for (int c = 0; c < d.ncomp; c++) {
      const int dct = d.dc_tbl[c], act = 4 + d.ac_tbl[c];
      for (int v = 0; v < d.vs[c]; v++)
        for (int h = 0; h < d.hs[c]; h++) {
          const int by = my * d.vs[c] + v, bx = mx * d.hs[c] + h;
          short* blk = coef + comp_base[c] + ((long long)by * d.bw[c] + bx) * 64;
          br.fill();
          const int s = huff_decode(br, t, dct);
          if (s < 0) return X3D_JPEG_CORRUPT;
          int diff = 0;
          if (s) {
            diff = extend(br.peek(s), s);
            br.skip(s);
          }
          pred[c] = (int)((unsigned)pred[c] + (unsigned)diff);   // wraps (int16 stores) on garbage, never UB
          blk[0] = (short)pred[c];
          for (int k = 1; k < 64; k++) {
            br.fill();
            const int rs = huff_decode(br, t, act);
            if (rs < 0) return X3D_JPEG_CORRUPT;
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
              k += r;
              const int val = extend(br.peek(sz), sz);
              br.skip(sz);
              blk[k > 63 ? 63 : kZigzag[k]] = (short)val;
            } else {
              if (r != 15) break;
              k += 15;
            }
          }
          if (br.used > br.real) return X3D_JPEG_CORRUPT;   // ran past the end of the segment
        }
    }
  }
  // what the scan left over must hold no marker: the host decoder skips other bytes on its way to EOI, but acts on a
  // marker (and fails on one it does not know).  br.p: the first byte not loaded, or the marker that stopped fill().
  for (const unsigned char* q = br.p; q + 1 < br.end; q++)
    if (q[0] == 0xFF && q[1] != 0x00 && q[1] != 0xFF) return X3D_JPEG_CORRUPT;
  return X3D_JPEG_OK;
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const unsigned char* __restrict__ data,
                                                         const x3d_jpeg_image* __restrict__ imgs, short* scratch,
                                                         int* status) {
  __shared__ HuffLds t;
  const int img = blockIdx.x;
  const x3d_jpeg_image& d = imgs[img];
  const int lane = threadIdx.x;
  if (d.status != X3D_JPEG_OK || d.out == nullptr) {
    if (lane == 0) status[img] = d.status != X3D_JPEG_OK ? d.status : X3D_JPEG_SKIPPED;
    return;
  }
  const unsigned char* base = data + d.data_off;
  if (lane < kTables) huff_limits(base, d, t, lane);
  __syncthreads();
  for (int e = lane; e < kTables << kLook; e += 64) huff_look(t, e);
  __syncthreads();
  if (lane == 0) status[img] = entropy_decode(base, d, t, scratch + d.coef_off / 2);
}

// ------------------------------------------------------------------------------------------------
// device: dequantise + ISLOW IDCT, one thread per block
// ------------------------------------------------------------------------------------------------
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
constexpr int kConstBits = 13, kPass1Bits = 2;

__host__ __device__ inline long long descale(long long x, int n) { return (x + (1ll << (n - 1))) >> n; }

// The range in which every build of the host decoder computes the same sample, and this file with them.  libjpeg limits
// the IDCT result v (before the + 128) through a table that holds the clamp for v in [-512, 511] and wraps beyond it; the
// SIMD builds of libjpeg-turbo dequantise and add in 16 bits, accumulate in 32 and saturate where they narrow.  Samples
// within [-512, 511] are the transform of coefficients within 6.6 x 512 (the largest 2-D basis sum, (5.13 / 2)^2) and of
// pass-1 values within 4 x 2.6 x 512 (the 1-D sum, scaled by 2^kPass1Bits): with 4095 and 16383 as the limits no legal
// block is refused that the sample range would not refuse, no 16-bit sum of two inputs wraps, and no sum of four
// products with the 15-bit constants leaves 32 bits.  A block outside them is damaged data: X3D_JPEG_CORRUPT.
constexpr int kCoefLimit = 4095, kPass1Limit = 16383, kSampleLo = -512, kSampleHi = 511;

// one 1-D 8-point pass over x[0], x[s], ..., x[7s]; results descaled by `sh` into y[0], y[t], ..., y[7t] (64-bit
// arithmetic: the garbage coefficients of a corrupt stream cannot overflow).  false: an input beyond +-in_lim or a
// descaled result outside [out_lo, out_hi] (see above).
template <typename In, typename Out>
__host__ __device__ inline bool idct_1d(const In* x, int s, Out* y, int t, int sh, const unsigned short* q, int add,
                                        int in_lim, int out_lo, int out_hi) {
  bool ok = true;
  auto in = [&](int k) {
    const long long v = q ? (long long)x[k * s] * q[k * s] : (long long)x[k * s];
    ok &= v >= -in_lim && v <= in_lim;
    return v;
  };
  long long z2 = in(2), z3 = in(6);
  long long z1 = (z2 + z3) * FIX_0_541196100;
  long long tmp2 = z1 + z3 * (-FIX_1_847759065);
  long long tmp3 = z1 + z2 * FIX_0_765366865;
  z2 = in(0);
  z3 = in(4);
  long long tmp0 = (z2 + z3) * (1 << kConstBits);
  long long tmp1 = (z2 - z3) * (1 << kConstBits);
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in(7);
  tmp1 = in(5);
  tmp2 = in(3);
  tmp3 = in(1);
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 *= -FIX_1_961570560;
  z4 *= -FIX_0_390180644;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  auto out = [&](int k, long long v) {
    v = descale(v, sh);
    ok &= v >= out_lo && v <= out_hi;
    v += add;
    if (add) v = v < 0 ? 0 : (v > 255 ? 255 : v);
    y[k * t] = (Out)v;
  };
  out(0, tmp10 + tmp3);
  out(7, tmp10 - tmp3);
  out(1, tmp11 + tmp2);
  out(6, tmp11 - tmp2);
  out(2, tmp12 + tmp1);
  out(5, tmp12 - tmp1);
  out(3, tmp13 + tmp0);
  out(4, tmp13 - tmp0);
  return ok;
}

// block b (over all components of the image, component-major) -> its 8x8 pixels in the component plane; false: the
// block's values leave the range in which the host decoders agree (the plane is written all the same)
__host__ __device__ inline bool idct_block(const x3d_jpeg_image& d, unsigned char* scratch, long long b) {
  int c = 0;
  long long cb = 0, pb = 0;                 // coefficient blocks / plane bytes of the components before c
  for (; c < d.ncomp; c++) {
    const long long nb = (long long)d.bw[c] * d.bh[c];
    if (b < nb) break;
    b -= nb;
    cb += nb;
    pb += nb * 64;
  }
  if (c >= d.ncomp) return true;
  const short* blk = (const short*)(scratch + d.coef_off) + (cb + b) * 64;
  const int stride = d.bw[c] * 8;
  const int by = (int)(b / d.bw[c]), bx = (int)(b % d.bw[c]);
  unsigned char* o = scratch + d.plane_off + pb + (long long)by * 8 * stride + bx * 8;
  short in[64];
  unsigned short q[64];
  for (int k = 0; k < 64; k++) { in[k] = blk[k]; q[k] = d.qt[c][k]; }
  int ws[64];
  bool ok = true;
  for (int col = 0; col < 8; col++)
    ok &= idct_1d(in + col, 8, ws + col, 8, kConstBits - kPass1Bits, q + col, 0, kCoefLimit, -kPass1Limit, kPass1Limit);
  unsigned char px[64];
  for (int row = 0; row < 8; row++)
    ok &= idct_1d(ws + row * 8, 1, px + row * 8, 1, kConstBits + kPass1Bits + 3, (const unsigned short*)nullptr, 128,
                  kPass1Limit, kSampleLo, kSampleHi);
  for (int row = 0; row < 8; row++) {
    unsigned long long v = 0;
    for (int k = 0; k < 8; k++) v |= (unsigned long long)px[row * 8 + k] << (8 * k);
    *(unsigned long long*)(o + (long long)row * stride) = v;
  }
  return ok;
}

// (a thread that finds its block out of range reports the image; the threads that race with the store read OK or
// CORRUPT there and do their block or not, and the colour launch, which comes after, sees CORRUPT.  Relaxed atomic
// accesses: the word is read and written by different threads of one launch on purpose.)
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const x3d_jpeg_image* __restrict__ imgs, unsigned char* scratch,
                                                       int* status) {
  int* st = status + blockIdx.y;
  if (__hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != X3D_JPEG_OK) return;
  if (!idct_block(imgs[blockIdx.y], scratch, (long long)blockIdx.x * 256 + threadIdx.x))
    __hip_atomic_store(st, X3D_JPEG_CORRUPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// device: upsample + colour conversion, one thread per output pixel
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline int chroma_at(const unsigned char* pl, int stride, int dw, int dh, int hr, int vr, int y, int x) {
  if (hr == 1) return pl[(long long)y * stride + x];
  const int j = x >> 1;
  if (dw <= 2) return pl[(long long)(vr == 2 ? y >> 1 : y) * stride + j];   // replication (no fancy upsampling)
  const int jl = j > 0 ? j - 1 : 0, jr = j < dw - 1 ? j + 1 : dw - 1;
  const int jn = (x & 1) ? jr : jl;
  if (vr == 1) {
    const unsigned char* r = pl + (long long)y * stride;
    return (x & 1) ? (3 * r[j] + r[jn] + 2) >> 2 : (3 * r[j] + r[jn] + 1) >> 2;
  }
  const int i = y >> 1;
  const int ifar = (y & 1) ? (i < dh - 1 ? i + 1 : dh - 1) : (i > 0 ? i - 1 : 0);
  const unsigned char* r0 = pl + (long long)i * stride;
  const unsigned char* r1 = pl + (long long)ifar * stride;
  const int cs = 3 * r0[j] + r1[j], cn = 3 * r0[jn] + r1[jn];
  return (x & 1) ? (3 * cs + cn + 7) >> 4 : (3 * cs + cn + 8) >> 4;
}

__host__ __device__ inline unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// output pixel i of the image
__host__ __device__ inline void color_pixel(const x3d_jpeg_image& d, const unsigned char* scratch, long long i) {
  if (i >= (long long)d.height * d.width) return;
  const int y = (int)(i / d.width), x = (int)(i % d.width);
  const unsigned char* pl = scratch + d.plane_off;
  const int s0 = d.bw[0] * 8;
  const int Y = pl[(long long)y * s0 + x];
  unsigned char* o = d.out + i * 3;
  if (d.ncomp == 1) {
    o[0] = o[1] = o[2] = (unsigned char)Y;
    return;
  }
  const unsigned char* pcb = pl + (long long)d.bw[0] * d.bh[0] * 64;
  const unsigned char* pcr = pcb + (long long)d.bw[1] * d.bh[1] * 64;
  const int s1 = d.bw[1] * 8;
  const int hr = d.hs[0], vr = d.vs[0];              // chroma is 1x1: the luma factors are the ratios
  const int dw = (d.width + hr - 1) / hr, dh = (d.height + vr - 1) / vr;
  const int cb = chroma_at(pcb, s1, dw, dh, hr, vr, y, x) - 128;
  const int cr = chroma_at(pcr, s1, dw, dh, hr, vr, y, x) - 128;
  // 16-bit fixed point: 1.40200, 1.77200, 0.71414, 0.34414 scaled by 2^16 and rounded
  const int r = (91881 * cr + 32768) >> 16;
  const int b = (116130 * cb + 32768) >> 16;
  const int g = (-46802 * cr + (-22554 * cb + 32768)) >> 16;
  o[0] = clamp255(Y + r);
  o[1] = clamp255(Y + g);
  o[2] = clamp255(Y + b);
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const x3d_jpeg_image* __restrict__ imgs,
                                                        const unsigned char* __restrict__ scratch,
                                                        const int* __restrict__ status) {
  if (status[blockIdx.y] != X3D_JPEG_OK) return;
  color_pixel(imgs[blockIdx.y], scratch, (long long)blockIdx.x * 256 + threadIdx.x);
}

}  // namespace

extern "C" int x3d_jpeg_decode(const x3d_jpeg_decode_args* a, void* stream) {
  X3D_REQUIRE(a && a->n >= 0, "jpeg_decode: bad arguments");
  if (a->n == 0) return X3D_OK;
  X3D_REQUIRE(a->data && a->images && a->host_images && a->status && (a->scratch || a->scratch_bytes == 0),
              "jpeg_decode: null pointer");
  X3D_REQUIRE(a->n < 65536, "jpeg_decode: %d images in one call (at most 65535)", a->n);
  long long coef_end = 0, max_blocks = 0, max_pix = 0;
  for (int i = 0; i < a->n; i++) {
    const x3d_jpeg_image* d = a->host_images + i;
    if (d->status != X3D_JPEG_OK) continue;
    const long long nb = blocks_of(d);
    X3D_REQUIRE(d->data_off >= 0 && d->data_len > 0 && d->ecs_off >= 0 && d->ecs_off <= d->ecs_end &&
                    d->ecs_end <= d->data_len,
                "jpeg_decode: image %d: entropy segment outside its bytes", i);
    X3D_REQUIRE(d->coef_off >= 0 && d->coef_off + nb * 128 <= d->plane_off && d->plane_off + nb * 64 <= a->scratch_bytes,
                "jpeg_decode: image %d: scratch layout exceeds the %lld-byte scratch", i, a->scratch_bytes);
    if (d->coef_off + nb * 128 > coef_end) coef_end = d->coef_off + nb * 128;
    if (nb > max_blocks) max_blocks = nb;
    const long long px = (long long)d->height * d->width;
    if (px > max_pix) max_pix = px;
  }
  hipStream_t st = (hipStream_t)stream;
  if (coef_end > 0 && hipMemsetAsync(a->scratch, 0, coef_end, st) != hipSuccess) {
    x3d_set_error("jpeg_decode: memset failed");
    return X3D_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(a->n), dim3(64), 0, st, a->data, a->images, (short*)a->scratch, a->status);
  X3D_LAUNCH_CHECK("jpeg_entropy");
  if (max_blocks > 0) {
    X3D_REQUIRE(ceil_div_ll(max_pix, 256) < (1ll << 31), "jpeg_decode: image too large");
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ceil_div_ll(max_blocks, 256), a->n), dim3(256), 0, st, a->images,
                       (unsigned char*)a->scratch, a->status);
    X3D_LAUNCH_CHECK("jpeg_idct");
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)ceil_div_ll(max_pix, 256), a->n), dim3(256), 0, st, a->images,
                       (const unsigned char*)a->scratch, a->status);
    X3D_LAUNCH_CHECK("jpeg_color");
  }
  return X3D_OK;
}
