// Baseline JPEG decoder (gfx950): JFIF files enter the GPU as bytes and leave as pixels, the inverse of jpeg.hip.
//
//   1. jpeg_decode_marks_kernel    flags FF D0..D7 in each file's scan (byte stuffing makes every such pair a marker), a
//                                  prefix sum writes marks[file][k] = where the k-th RSTn stands; a count other than the
//                                  file's intervals - 1 sets a status bit
//   2. jpeg_decode_entropy_kernel  one lane per restart interval, the file's Huffman tables in LDS: a 9-bit first-level
//                                  lookup, the canonical maxcode / valptr walk for longer codes, a 64-bit bit buffer with
//                                  FF 00 unstuffed; non-zero coefficients go as int16, zigzagged, into a zero-filled
//                                  [N][blocks][64] buffer in MCU scan order
//   3. jpeg_decode_idct_kernel     dequantise, the exact integer IDCT, u8 component planes (padded to whole MCUs)
//   4. jpeg_decode_colour_kernel   "fancy" chroma upsampling over the component's true size, 16.16 YCbCr -> RGB, the
//                                  output layout and type
//
// The definition of every number is self_forcing_amd/jpeg_reference.py (`parse`, `decode_coefficients`, `decode`); the
// kernels equal it bit for bit.  The host side of the caller reads the header segments only and uploads, in one copy, a
// table block (one JpegDecFile per file) followed by the files' bytes.  Every loop below is bounded by the interval's
// block count and byte range, every read is clamped to the upload, every write to the call's geometry: a damaged file
// sets bits of its status word and leaves zeros, it cannot reach another file's memory.
#include "sf_frame_host.h"
#include "pixel_format.h"

namespace {

constexpr int LOOK_BITS = 9;
// jpeg_reference.decode_tables: look[next 9 bits] = (length << 8) | symbol, 0 for a longer code; a code of length L > 9 is
// the first L whose next L bits are <= maxcode[L], its symbol vals[code + valoff[L]]
struct JpegDecHuff {
  uint16_t look[1 << LOOK_BITS];
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t vals[256];
};
// one file's entry of the table block (little endian, as _jpeg_decode_tables packs it)
struct JpegDecFile {
  uint32_t scan_off, scan_len;     // the entropy-coded bytes: upload[scan_off .. scan_off + scan_len)
  uint32_t ri, intervals;          // MCUs per restart interval (the MCU count without DRI), ceil(MCUs / ri)
  uint16_t quant[3][64];           // per component, natural order
  JpegDecHuff huff[3][2];          // per component: DC, AC
  uint8_t pad[16];
};
static_assert(sizeof(JpegDecHuff) == 1424 && sizeof(JpegDecFile) == SF_JPEG_DECODE_FILE_BYTES, "the table block's layout is part of the ABI");
constexpr int HUFF_WORDS = (int)(6 * sizeof(JpegDecHuff) / 4);

struct IdctTable { int32_t bi[64]; uint8_t zz[64]; };              // bi[k * 8 + n] = rint(2^13 b(k, n)); zz = kZigzag

struct DecGeometry {
  int comps, bpm, lbx, lby;        // components, blocks per MCU, luma blocks across / down one MCU
  int mcus_x, mcus_y, mcus, blocks;
  int yw, yh, cw, ch;              // padded plane sizes of luma and chroma
  int tcw, tch;                    // the chroma components' true size: ceil(w / lbx), ceil(h / lby)
  size_t marks_off, counts_off, coef_off, plane_off[3], total;
};

int geometry(const char* who, int n, int h, int w, int sampling, int max_intervals, DecGeometry* g) {
  SF_CHECK(sampling >= SF_JPEG_DEC_420 && sampling <= SF_JPEG_DEC_GRAY, "%s: unknown sampling %d", who, sampling);
  SF_CHECK(n > 0 && n <= 65535, "%s: n=%d files (1..65535)", who, n);
  SF_CHECK(h > 0 && w > 0 && h <= 65535 && w <= 65535, "%s: frame %dx%d (1..65535)", who, h, w);
  g->comps = sampling == SF_JPEG_DEC_GRAY ? 1 : 3;
  g->lbx = sampling == SF_JPEG_DEC_420 || sampling == SF_JPEG_DEC_422 ? 2 : 1;
  g->lby = sampling == SF_JPEG_DEC_420 ? 2 : 1;
  g->bpm = g->lbx * g->lby + (g->comps == 3 ? 2 : 0);
  g->mcus_x = (w + 8 * g->lbx - 1) / (8 * g->lbx);
  g->mcus_y = (h + 8 * g->lby - 1) / (8 * g->lby);
  SF_CHECK((long)g->mcus_x * g->mcus_y * g->bpm <= (1 << 26), "%s: frame %dx%d has more than 2^26 blocks", who, h, w);
  g->mcus = g->mcus_x * g->mcus_y;
  g->blocks = g->mcus * g->bpm;
  SF_CHECK(max_intervals >= 1 && max_intervals <= g->mcus, "%s: max_intervals=%d (1..%d MCUs)", who, max_intervals, g->mcus);
  g->yw = g->mcus_x * g->lbx * 8, g->yh = g->mcus_y * g->lby * 8;
  g->cw = g->mcus_x * 8, g->ch = g->mcus_y * 8;
  g->tcw = (w + g->lbx - 1) / g->lbx, g->tch = (h + g->lby - 1) / g->lby;
  size_t off = 0;                                                  // (the marker table last: nothing in front of it depends on max_intervals)
  g->coef_off = off, off += align256((size_t)n * g->blocks * 128);
  g->plane_off[0] = off, off += align256((size_t)n * g->yw * g->yh);
  for (int c = 1; c < 3; ++c) g->plane_off[c] = off, off += g->comps == 3 ? align256((size_t)n * g->cw * g->ch) : 0;
  g->counts_off = off, off += align256((size_t)n * 4);
  g->marks_off = off, off += align256((size_t)n * max_intervals * 4);
  g->total = off;
  return 0;
}

int check_upload(const char* who, const void* upload, size_t upload_bytes, int n) {
  SF_CHECK(upload && (uintptr_t)upload % 16 == 0 && upload_bytes % 16 == 0, "%s: upload must be a 16-byte-aligned buffer of a multiple of 16 bytes", who);
  SF_CHECK(upload_bytes >= (size_t)n * sizeof(JpegDecFile) && upload_bytes < 0x7FFFFFF0u, "%s: upload of %zu bytes cannot hold %d table entries (or exceeds 2 GiB)",
           who, upload_bytes, n);
  return 0;
}

// the file's scan as [off, end) of the upload, clamped to it
__device__ __forceinline__ void scan_range(const JpegDecFile* d, uint32_t upload_bytes, uint32_t& off, uint32_t& end) {
  off = d->scan_off < upload_bytes ? d->scan_off : upload_bytes;
  const uint32_t len = d->scan_len < upload_bytes - off ? d->scan_len : upload_bytes - off;
  end = off + len;
}

// ------------------------------------------------------------------------------------------------ restart search
// grid N x 256: 16 bytes per thread and step.  marks[f][k] = offset (inside the scan) of the k-th RSTn marker, counts[f] =
// how many there are (only the first max_intervals are stored).
__global__ __launch_bounds__(256) void jpeg_decode_marks_kernel(const uint8_t* __restrict__ up, uint32_t upload_bytes, uint32_t* __restrict__ marks,
                                                                uint32_t* __restrict__ counts, int32_t* __restrict__ status, int max_intervals) {
  __shared__ uint32_t s[256];
  const int t = threadIdx.x;
  const long f = blockIdx.x;
  const JpegDecFile* d = (const JpegDecFile*)(up + f * sizeof(JpegDecFile));
  uint32_t off, end;
  scan_range(d, upload_bytes, off, end);
  uint32_t running = 0;
  for (uint32_t a0 = off & ~15u; a0 < end; a0 += 256 * 16) {
    const uint32_t a = a0 + (uint32_t)t * 16;
    uint32_t mask = 0;                                           // bit j: a marker stands at byte a + j
    if (a < end) {                                               // a + 16 <= upload_bytes: both are multiples of 16
      const u32x4 v = *(const u32x4*)(up + a);
      const uint32_t after = a + 16 < end ? up[a + 16] : 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t b0 = (v[j >> 2] >> (8 * (j & 3))) & 255u;
        const uint32_t b1 = j < 15 ? (v[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u : after;
        const uint32_t pos = a + j;
        if (pos >= off && pos + 1 < end && b0 == 0xFFu && (b1 & 0xF8u) == 0xD0u) mask |= 1u << j;
      }
    }
    const uint32_t mine = __popc(mask);
    s[t] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const uint32_t x = t >= o ? s[t - o] : 0u;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    uint32_t idx = running + s[t] - mine;
    for (uint32_t m = mask; m; m &= m - 1, ++idx)
      if (idx < (uint32_t)max_intervals) marks[f * max_intervals + idx] = a + (uint32_t)(__ffs(m) - 1) - off;
    running += s[255];
    __syncthreads();
  }
  if (t == 0) {
    counts[f] = running;
    if (running + 1u != d->intervals) atomicOr(&status[f], SF_JPEG_DEC_MARKER_COUNT);
  }
}

// ------------------------------------------------------------------------------------------------ entropy decoding
struct BitReader {
  const uint8_t* up;
  uint32_t pos, end;               // the interval's bytes: upload[pos .. end)
  uint64_t acc;
  int n, phantom;                  // bits in acc; how many of the bits shifted in so far lay behind `end` (zeros)
  u32x4 word;                      // the aligned 16 bytes last loaded (inside the upload: its size is a multiple of 16)
  uint32_t word_at;                // and their byte offset: a lane waits for memory once per 16 bytes, not once per 4
  __device__ __forceinline__ uint32_t byte_at(uint32_t p) {
    if ((p & ~15u) != word_at) word_at = p & ~15u, word = *(const u32x4*)(up + word_at);
    const uint32_t lo = (p & 4u) ? word.y : word.x, hi = (p & 4u) ? word.w : word.z;
    return (((p & 8u) ? hi : lo) >> (8 * (p & 3u))) & 255u;
  }
  // at least 57 bits afterwards: enough for a code (16) and its extra bits (15)
  __device__ __forceinline__ void fill() {
    while (n <= 56) {
      uint32_t b = 0;
      if (pos < end) {
        b = byte_at(pos++);
        if (b == 0xFFu && pos < end && byte_at(pos) == 0u) ++pos;          // FF 00 is a stuffed FF
      } else if (phantom < (1 << 20)) {
        phantom += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  __device__ __forceinline__ uint32_t peek(int len) const { return (uint32_t)(acc >> (n - len)) & ((1u << len) - 1u); }
  __device__ __forceinline__ void skip(int len) { n -= len; }
  // T.81 F.2.2.1 EXTEND of the next `size` bits (1..15)
  __device__ __forceinline__ int receive(int size) {
    const int v = (int)peek(size);
    skip(size);
    return v >> (size - 1) ? v : v - (1 << size) + 1;
  }
  __device__ __forceinline__ bool overrun() const { return n < phantom; }
};

// the next symbol, -1 for a bit pattern that is no code
__device__ __forceinline__ int huff_symbol(BitReader& br, const JpegDecHuff& h) {
  const uint32_t e = h.look[br.peek(LOOK_BITS)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int len = LOOK_BITS + 1; len <= 16; ++len) {
    const int code = (int)br.peek(len);
    if (code <= h.maxcode[len]) {
      br.skip(len);
      return (int)h.vals[(code + h.valoff[len]) & 255];
    }
  }
  return -1;
}

// grid (ceil(max_intervals / 64), N) x 64: one lane per restart interval, all lanes of a workgroup in one file
__global__ __launch_bounds__(64) void jpeg_decode_entropy_kernel(const uint8_t* __restrict__ up, uint32_t upload_bytes, const uint32_t* __restrict__ marks,
                                                                 const uint32_t* __restrict__ counts, int16_t* __restrict__ coef, int32_t* __restrict__ status,
                                                                 int max_intervals, int bpm, int mcus, int blocks_per_frame) {
  __shared__ JpegDecHuff sHuff[3][2];
  const int lane = threadIdx.x;
  const long f = blockIdx.y;
  const JpegDecFile* d = (const JpegDecFile*)(up + f * sizeof(JpegDecFile));
  {
    const uint32_t* src = (const uint32_t*)&d->huff[0][0];
    uint32_t* dst = (uint32_t*)&sHuff[0][0];
    for (int i = lane; i < HUFF_WORDS; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  const long iv = (long)blockIdx.x * 64 + lane;
  const long ri = d->ri ? d->ri : 1;
  const long intervals = d->intervals < (uint32_t)max_intervals ? d->intervals : max_intervals;
  if (iv >= intervals || iv * ri >= mcus) return;
  const int block0 = (int)(iv * ri) * bpm;
  const int nblocks = (int)(ri < mcus - iv * ri ? ri : mcus - iv * ri) * bpm;
  uint32_t off, end;
  scan_range(d, upload_bytes, off, end);
  const uint32_t nmarks = counts[f] < (uint32_t)max_intervals ? counts[f] : max_intervals;
  if (iv > nmarks) {                                               // the file holds no such interval (its marker count is flagged)
    atomicOr(&status[f], SF_JPEG_DEC_TRUNCATED);
    return;
  }
  const uint32_t* mk = marks + f * max_intervals;
  uint32_t a = iv == 0 ? off : off + mk[iv - 1] + 2, b = iv < nmarks ? off + mk[iv] : end;
  if (b > end) b = end;
  if (a > b) a = b;
  BitReader br{up, a, b, 0, 0, 0, u32x4{0, 0, 0, 0}, 0xFFFFFFFFu};
  int16_t* out = coef + ((long)f * blocks_per_frame + block0) * 64;
  int pred[3] = {0, 0, 0};
  int flags = 0;
  for (int j = 0; j < nblocks && !flags; ++j, out += 64) {
    const int k = j % bpm;
    const int comp = bpm == 1 ? 0 : (k < bpm - 2 ? 0 : k - (bpm - 3));
    br.fill();
    const int size = huff_symbol(br, sHuff[comp][0]);
    if (size < 0 || size > 11) {
      flags |= SF_JPEG_DEC_BAD_CODE;
      break;
    }
    if (size) pred[comp] += br.receive(size);
    if (pred[comp]) out[0] = (int16_t)pred[comp];
    for (int pos = 1; pos < 64;) {
      br.fill();
      const int rs = huff_symbol(br, sHuff[comp][1]);
      if (rs < 0) {
        flags |= SF_JPEG_DEC_BAD_CODE;
        break;
      }
      const int run = rs >> 4, sz = rs & 15;
      if (sz == 0) {
        if (run != 15) break;                                      // EOB
        pos += 16;                                                 // ZRL
        continue;
      }
      pos += run;
      if (pos > 63) {
        flags |= SF_JPEG_DEC_RUN_PAST_63;
        break;
      }
      out[pos] = (int16_t)br.receive(sz);
      ++pos;
    }
    if (br.overrun()) flags |= SF_JPEG_DEC_TRUNCATED;
  }
  if (flags) atomicOr(&status[f], flags);
}

// ------------------------------------------------------------------------------------------------ IDCT
// grid (ceil(blocks / 32), N) x 256: eight threads per block.  X = coef * Q in natural order, u = Bi^T X by columns, t = u Bi
// by rows, all exact in 64 bits; sample = clamp(((t + 2^25) >> 26) + 128, 0, 255).
__global__ __launch_bounds__(256) void jpeg_decode_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ up, uint8_t* __restrict__ plane_y,
                                                               uint8_t* __restrict__ plane_cb, uint8_t* __restrict__ plane_cr, const IdctTable tab, int bpm, int lbx,
                                                               int mcus_x, int blocks_per_frame, int yw, int yh, int cw, int ch) {
  __shared__ int32_t sX[32][64];
  __shared__ int64_t sU[32][64];
  const int t = threadIdx.x, b = t >> 3, j = t & 7;
  const long f = blockIdx.y;
  const int blk = blockIdx.x * 32 + b;
  const bool live = blk < blocks_per_frame;
  const JpegDecFile* d = (const JpegDecFile*)(up + f * sizeof(JpegDecFile));
  const int m = blk / bpm, k = blk - m * bpm;
  const int comp = bpm == 1 ? 0 : (k < bpm - 2 ? 0 : k - (bpm - 3));
  if (live) {
    const u32x4 raw = *(const u32x4*)(coef + ((long)f * blocks_per_frame + blk) * 64 + j * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = (int)(int16_t)(raw[i >> 1] >> ((i & 1) * 16));
      const int nat = tab.zz[j * 8 + i];
      sX[b][nat] = v * (int)d->quant[comp][nat];
    }
  }
  __syncthreads();
  if (live) {                                                      // column j: u[n][j] = sum_k Bi[k][n] X[k][j]
    int x[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) x[kk] = sX[b][kk * 8 + j];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      int64_t acc = 0;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) acc += (int64_t)tab.bi[kk * 8 + n] * x[kk];
      sU[b][n * 8 + j] = acc;
    }
  }
  __syncthreads();
  if (live) {                                                      // row j: t[j][mm] = sum_i u[j][i] Bi[i][mm]
    int64_t u[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) u[i] = sU[b][j * 8 + i];
    uint32_t packed[2] = {0, 0};
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {
      int64_t acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += u[i] * (int64_t)tab.bi[i * 8 + mm];
      int64_t s = ((acc + ((int64_t)1 << 25)) >> 26) + 128;
      s = s < 0 ? 0 : (s > 255 ? 255 : s);
      packed[mm >> 2] |= (uint32_t)s << (8 * (mm & 3));
    }
    const int mx = m % mcus_x, my = m / mcus_x;
    uint8_t* dst;
    if (comp == 0) {
      const int lby = (bpm == 1 ? 1 : bpm - 2) / lbx;              // the MCU's luma blocks: lbx across, lby down
      const int bx = mx * lbx + k % lbx, by = my * lby + k / lbx;
      dst = plane_y + ((long)f * yh + by * 8 + j) * yw + bx * 8;
    } else {
      dst = (comp == 1 ? plane_cb : plane_cr) + ((long)f * ch + my * 8 + j) * cw + mx * 8;
    }
    *(u32x2*)dst = u32x2{packed[0], packed[1]};
  }
}

// ------------------------------------------------------------------------------------------------ upsampling, colour, format
constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }
constexpr int FIX_CR_R = fix16(1.402), FIX_CB_G = fix16(0.344136286), FIX_CR_G = fix16(0.714136286), FIX_CB_B = fix16(1.772);

// the chroma plane `p` (rows of `ld`) at output pixels x0 .. x0 + 3 of row y: libjpeg's triangle filter over the
// component's true size tcw x tch, edges replicated (jpeg_reference.upsample)
__device__ __forceinline__ void chroma4(const uint8_t* __restrict__ p, int ld, int lbx, int lby, int tcw, int tch, int x0, int y, int (&c)[4]) {
  if (lbx == 1) {
    const uint32_t v = *(const uint32_t*)(p + (long)y * ld + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (int)((v >> (8 * i)) & 255u);
    return;
  }
  const int cx = x0 >> 1;
  int xs[4] = {cx - 1, cx, cx + 1, cx + 2};
#pragma unroll
  for (int i = 0; i < 4; ++i) xs[i] = xs[i] < 0 ? 0 : (xs[i] > tcw - 1 ? tcw - 1 : xs[i]);
  int t[4];
  if (lby == 2) {
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > tch - 1 ? tch - 1 : fy);
    const uint8_t *near = p + (long)cy * ld, *far = p + (long)fy * ld;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = 3 * (int)near[xs[i]] + (int)far[xs[i]];
    c[0] = (3 * t[1] + t[0] + 8) >> 4;
    c[1] = (3 * t[1] + t[2] + 7) >> 4;
    c[2] = (3 * t[2] + t[1] + 8) >> 4;
    c[3] = (3 * t[2] + t[3] + 7) >> 4;
  } else {
    const uint8_t* row = p + (long)y * ld;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = (int)row[xs[i]];
    c[0] = (3 * t[1] + t[0] + 1) >> 2;
    c[1] = (3 * t[1] + t[2] + 2) >> 2;
    c[2] = (3 * t[2] + t[1] + 1) >> 2;
    c[3] = (3 * t[2] + t[3] + 2) >> 2;
  }
}

// grid (ceil(ceil(W / 4) / 64), ceil(H / 4), N) x (64, 4): four pixels of one row per thread.  Element (f, c, y, x) of the
// output stands at f sn + c sc + y sy + x sx.
template <typename T>
__global__ __launch_bounds__(256) void jpeg_decode_colour_kernel(const uint8_t* __restrict__ plane_y, const uint8_t* __restrict__ plane_cb,
                                                                 const uint8_t* __restrict__ plane_cr, T* __restrict__ out, int H, int W, int comps, int lbx, int lby,
                                                                 int yw, int yh, int cw, int ch, int tcw, int tch, long sn, long sc, long sy, long sx) {
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
  const long f = blockIdx.z;
  if (x0 >= W || y >= H) return;
  int rgb[3][4];
  {
    const uint32_t v = *(const uint32_t*)(plane_y + ((long)f * yh + y) * yw + x0);     // x0 + 3 < yw: yw is a multiple of 8
#pragma unroll
    for (int i = 0; i < 4; ++i) rgb[0][i] = (int)((v >> (8 * i)) & 255u);
  }
  if (comps == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rgb[1][i] = rgb[2][i] = rgb[0][i];
  } else {
    int cb[4], cr[4];
    chroma4(plane_cb + (long)f * ch * cw, cw, lbx, lby, tcw, tch, x0, y, cb);
    chroma4(plane_cr + (long)f * ch * cw, cw, lbx, lby, tcw, tch, x0, y, cr);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int yy = rgb[0][i], u = cb[i] - 128, v = cr[i] - 128;
      rgb[0][i] = clamp255(yy + ((FIX_CR_R * v + 32768) >> 16));
      rgb[1][i] = clamp255(yy + ((-FIX_CB_G * u - FIX_CR_G * v + 32768) >> 16));
      rgb[2][i] = clamp255(yy + ((FIX_CB_B * u + 32768) >> 16));
    }
  }
  T* o = out + f * sn + (long)y * sy + (long)x0 * sx;
  store_rgb4(o, rgb, x0, W, sc, sx);
}

int launch_entropy(const char* who, const DecGeometry& g, const void* upload, size_t upload_bytes, int n, int max_intervals, char* ws, void* coef,
                   int32_t* status, hipStream_t s) {
  uint32_t* marks = (uint32_t*)(ws + g.marks_off);
  uint32_t* counts = (uint32_t*)(ws + g.counts_off);
  SF_TRY(sf_hip_ok(hipMemsetAsync(status, 0, (size_t)n * 4, s), who, "clearing the status words"));
  SF_TRY(sf_hip_ok(hipMemsetAsync(coef, 0, (size_t)n * g.blocks * 128, s), who, "clearing the coefficients"));
  SF_TRY(sf_launch<&jpeg_decode_marks_kernel>(who, dim3((unsigned)n), dim3(256), 0, s, (const uint8_t*)upload, (uint32_t)upload_bytes, marks, counts, status,
                                              max_intervals));
  return sf_launch<&jpeg_decode_entropy_kernel>(who, dim3((unsigned)((max_intervals + 63) / 64), (unsigned)n), dim3(64), 0, s, (const uint8_t*)upload,
                                                (uint32_t)upload_bytes, marks, counts, (int16_t*)coef, status, max_intervals, g.bpm, g.mcus, g.blocks);
}

}  // namespace

extern "C" size_t sf_jpeg_decode_workspace_bytes(int n, int h, int w, int sampling, int max_intervals) {
  DecGeometry g;
  if (geometry("sf_jpeg_decode_workspace_bytes", n, h, w, sampling, max_intervals, &g) != 0) return 0;
  return g.total;
}

extern "C" int sf_jpeg_decode_entropy(const void* upload, size_t upload_bytes, int n, int h, int w, int sampling, int max_intervals, void* workspace,
                                      size_t workspace_bytes, void* coef, int32_t* status, void* stream) {
  const char* who = "sf_jpeg_decode_entropy";
  DecGeometry g;
  SF_TRY(geometry(who, n, h, w, sampling, max_intervals, &g));
  SF_TRY(check_upload(who, upload, upload_bytes, n));
  SF_CHECK(workspace && coef && status, "%s: null buffer", who);
  SF_CHECK((uintptr_t)workspace % 256 == 0 && (uintptr_t)coef % 16 == 0 && (uintptr_t)status % 4 == 0,
           "%s: workspace must be 256-byte, coef 16-byte, status 4-byte aligned", who);
  SF_CHECK(workspace_bytes >= g.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g.total);
  return launch_entropy(who, g, upload, upload_bytes, n, max_intervals, (char*)workspace, coef, status, (hipStream_t)stream);
}

extern "C" int sf_jpeg_decode_pixels(const void* coef, const void* upload, size_t upload_bytes, const int32_t* idct_table, int n, int h, int w, int sampling,
                                     void* workspace, size_t workspace_bytes, void* out, int layout, int dtype, void* stream) {
  const char* who = "sf_jpeg_decode_pixels";
  DecGeometry g;
  SF_TRY(geometry(who, n, h, w, sampling, 1, &g));
  SF_TRY(check_upload(who, upload, upload_bytes, n));
  SF_CHECK(coef && workspace && out && idct_table, "%s: null buffer", who);
  SF_CHECK(layout >= SF_JPEG_HWC && layout <= SF_JPEG_CHW, "%s: unknown layout %d", who, layout);
  SF_CHECK(dtype >= SF_JPEG_U8 && dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK((uintptr_t)workspace % 256 == 0 && (uintptr_t)coef % 16 == 0 && (uintptr_t)out % 16 == 0,
           "%s: workspace must be 256-byte, coef and out 16-byte aligned", who);
  SF_CHECK(workspace_bytes >= g.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g.total);
  IdctTable tab;
  for (int i = 0; i < 64; ++i) {
    SF_CHECK(idct_table[i] >= -(1 << 13) && idct_table[i] <= (1 << 13), "%s: idct_table[%d]=%d is no 13-bit basis value", who, i, idct_table[i]);
    tab.bi[i] = idct_table[i];
    tab.zz[i] = kZigzag[i];
  }
  char* ws = (char*)workspace;
  uint8_t *py = (uint8_t*)(ws + g.plane_off[0]), *pcb = (uint8_t*)(ws + g.plane_off[1]), *pcr = (uint8_t*)(ws + g.plane_off[2]);
  hipStream_t s = (hipStream_t)stream;
  SF_TRY(sf_launch<&jpeg_decode_idct_kernel>(who, dim3((unsigned)((g.blocks + 31) / 32), (unsigned)n), dim3(256), 0, s, (const int16_t*)coef,
                                             (const uint8_t*)upload, py, pcb, pcr, tab, g.bpm, g.lbx, g.mcus_x, g.blocks, g.yw, g.yh, g.cw, g.ch));
  const FrameStrides to = frame_strides(layout, n, h, w);
  const dim3 grid((unsigned)(((w + 3) / 4 + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)n), block(64, 4);
  return pixel_dispatch(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return sf_launch<&jpeg_decode_colour_kernel<T>>(who, grid, block, 0, s, py, pcb, pcr, (T*)out, h, w, g.comps, g.lbx, g.lby, g.yw, g.yh, g.cw, g.ch,
                                                    g.tcw, g.tch, to.sn, to.sc, to.sy, to.sx);
  });
}

extern "C" int sf_jpeg_decode_frames(const void* upload, size_t upload_bytes, const int32_t* idct_table, int n, int h, int w, int sampling, int max_intervals,
                                     void* workspace, size_t workspace_bytes, void* out, int layout, int dtype, int32_t* status, void* stream) {
  const char* who = "sf_jpeg_decode_frames";
  DecGeometry g;
  SF_TRY(geometry(who, n, h, w, sampling, max_intervals, &g));
  SF_CHECK(workspace && (uintptr_t)workspace % 256 == 0, "%s: workspace must be 256-byte aligned", who);
  SF_CHECK(workspace_bytes >= g.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g.total);
  void* coef = (char*)workspace + g.coef_off;
  SF_TRY(sf_jpeg_decode_entropy(upload, upload_bytes, n, h, w, sampling, max_intervals, workspace, workspace_bytes, coef, status, stream));
  return sf_jpeg_decode_pixels(coef, upload, upload_bytes, idct_table, n, h, w, sampling, workspace, workspace_bytes, out, layout, dtype, stream);
}
