// Baseline JPEG encoder for decoded frames (gfx950): frames leave the GPU as JFIF files instead of fp32 pixels.
//
//   1. jpeg_transform_kernel   frames (fp32 / bf16 planar, or uint8 HWC) -> u8 truncation -> YCbCr -> (2x2 chroma mean) -> 8x8
//                              DCT -> quantise -> zigzag -> int16 [N][blocks][64] in MCU scan order
//   2. jpeg_entropy_kernel     one wave per restart interval: every lane Huffman-codes whole blocks into a private LDS slot,
//                              a wave prefix sum over the bit counts places them, ds_or merges them at bit granularity, the
//                              bytes are stuffed and written to the interval's own worst-case-sized slot
//   3. jpeg_scan_* / jpeg_pack_kernel   prefix sums over the interval lengths, then header + intervals + RSTn / EOI markers
//                              into one contiguous byte buffer, offsets[N + 1]
//
// The format and the definition of every number are those of self_forcing_amd/jpeg_reference.py (the float64 host oracle).
// Tables and the header travel as kernel arguments: the library uploads nothing and keeps no state.
#include "sf_frame_host.h"

namespace {

// ------------------------------------------------------------------------------------------------ tables (T.81 Annex K)
const uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
     0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
     0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
     0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
     0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
     0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};

constexpr int HDR_MAX = 640;                     // the header is 629 bytes
struct JpegHeader { uint8_t b[HDR_MAX]; int32_t len; };
struct QuantTables { float q[2][64]; uint8_t izz[64]; };          // natural order; izz[natural] = scan position
struct HuffTables { uint32_t t[2 * 16 + 2 * 256]; };             // (length << 16) | code: DC luma, DC chroma, AC luma, AC chroma
constexpr int HUFF_DC = 0, HUFF_AC = 32;

struct Geometry {
  int mcu, bpm, mcus_x, mcus_y, mcus, blocks, intervals, interval_blocks;
  size_t slot_bytes, coef_bytes, slots_off, lens_off, ipos_off, fsize_off, total;
};

// worst case of one block: the DC symbol (11 + 11 bits, chroma) and 63 AC symbols of 16 + 10 bits
constexpr int BLOCK_MAX_BITS = 22 + 63 * 26;                       // 1660
constexpr int BLOCK_MAX_BYTES = (BLOCK_MAX_BITS + 7) / 8;          // 208
constexpr int SLOT_DW = 53;                                        // 52 dwords hold it; odd stride: lanes hit distinct banks
constexpr int MERGE_DW = (64 * BLOCK_MAX_BITS + 7 + 31) / 32 + 2;  // one chunk of 64 blocks plus the carried bits

int quant_value(int base, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

int geometry(const char* who, int n, int h, int w, int sub, int ri, Geometry* g) {
  SF_CHECK(sub == SF_JPEG_420 || sub == SF_JPEG_444, "%s: unknown subsampling %d", who, sub);
  g->mcu = sub == SF_JPEG_420 ? 16 : 8;
  g->bpm = sub == SF_JPEG_420 ? 6 : 3;
  SF_CHECK(n > 0 && n <= 65535, "%s: n=%d frames (1..65535)", who, n);
  SF_CHECK(h > 0 && w > 0 && h <= 65535 && w <= 65535 && h % g->mcu == 0 && w % g->mcu == 0,
           "%s: frame %dx%d is not a multiple of the %dx%d MCU", who, h, w, g->mcu, g->mcu);
  SF_CHECK(ri >= 1 && ri <= 65535, "%s: restart_interval=%d (1..65535)", who, ri);
  g->mcus_x = w / g->mcu;
  g->mcus_y = h / g->mcu;
  g->mcus = g->mcus_x * g->mcus_y;
  g->blocks = g->mcus * g->bpm;
  g->intervals = (g->mcus + ri - 1) / ri;
  g->interval_blocks = (ri < g->mcus ? ri : g->mcus) * g->bpm;
  g->slot_bytes = ((size_t)g->interval_blocks * BLOCK_MAX_BYTES * 2 + 15) & ~(size_t)15;   // every byte stuffed
  g->coef_bytes = align256((size_t)n * g->blocks * 128);
  g->slots_off = g->coef_bytes;
  g->lens_off = g->slots_off + align256((size_t)n * g->intervals * g->slot_bytes);
  g->ipos_off = g->lens_off + align256((size_t)n * g->intervals * 4);
  g->fsize_off = g->ipos_off + align256((size_t)n * g->intervals * 4);
  g->total = g->fsize_off + align256((size_t)n * (4 + HDR_MAX));   // (+ a header per frame: `total` bytes always hold the files)
  return 0;
}

void huffman_table(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

uint8_t* put_segment(uint8_t* p, int marker, const uint8_t* payload, int n) {
  *p++ = 0xFF;
  *p++ = (uint8_t)marker;
  *p++ = (uint8_t)((n + 2) >> 8);
  *p++ = (uint8_t)(n + 2);
  for (int i = 0; i < n; ++i) *p++ = payload[i];
  return p;
}

// SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS: jpeg_reference.header
void build_header(int h, int w, int quality, int sub, int ri, JpegHeader* hd) {
  uint8_t* p = hd->b;
  uint8_t buf[200];
  *p++ = 0xFF;
  *p++ = 0xD8;
  const uint8_t app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p = put_segment(p, 0xE0, app0, 14);
  for (int t = 0; t < 2; ++t) {
    buf[0] = (uint8_t)t;
    for (int k = 0; k < 64; ++k) buf[1 + k] = (uint8_t)quant_value(kBaseQuant[t][kZigzag[k]], quality);
    p = put_segment(p, 0xDB, buf, 65);
  }
  const uint8_t sof[15] = {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3, 1, (uint8_t)(sub == SF_JPEG_420 ? 0x22 : 0x11), 0,
                           2, 0x11, 1, 3, 0x11, 1};
  p = put_segment(p, 0xC0, sof, 15);
  for (int t = 0; t < 2; ++t) {
    buf[0] = (uint8_t)t;
    for (int i = 0; i < 16; ++i) buf[1 + i] = kDcBits[t][i];
    for (int i = 0; i < 12; ++i) buf[17 + i] = kDcVals[i];
    p = put_segment(p, 0xC4, buf, 29);
    buf[0] = (uint8_t)(0x10 | t);
    for (int i = 0; i < 16; ++i) buf[1 + i] = kAcBits[t][i];
    for (int i = 0; i < 162; ++i) buf[17 + i] = kAcVals[t][i];
    p = put_segment(p, 0xC4, buf, 179);
  }
  const uint8_t dri[2] = {(uint8_t)(ri >> 8), (uint8_t)ri};
  p = put_segment(p, 0xDD, dri, 2);
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  p = put_segment(p, 0xDA, sos, 10);
  hd->len = (int32_t)(p - hd->b);
}

// ------------------------------------------------------------------------------------------------ transform
constexpr int TILE_W = 64;        // pixels per workgroup along x: 4 MCUs of "420", 8 of "444" -> 24 blocks either way
constexpr int TILE_BLOCKS = 24;
constexpr int PLANE_LD = 68;      // values per staged row (64 + padding)
constexpr int T_LD = 9, T_BLOCK = 72;

// Colour conversion, DCT and quantisation run in fp64 (full rate on CDNA; the kernel is bound by its loads).  In fp32
// about 1e-5 of the quotients c / Q at quality 100 land on the other side of a rounding tie than the float64 reference
// (numpy in fp32 against float64 on 480x832 noise frames: 9 of 1.2 M), and one such coefficient is already more than
// 1e-4 of a 16x16 frame's 768.
// D[k][n] = c(k) / 2 cos((2n + 1) k pi / 16): cos(j pi / 16) / 2 for j = 1..7, and 1 / (2 sqrt 2)
#define SF_C1 0.49039264020161522456
#define SF_C2 0.46193976625564337806
#define SF_C3 0.41573480615127261854
#define SF_C4 0.35355339059327376220
#define SF_C5 0.27778511650980111237
#define SF_C6 0.19134171618254488586
#define SF_C7 0.09754516100806413392

__device__ __forceinline__ void dct8(const double (&x)[8], double (&o)[8]) {
  constexpr double D[8][8] = {{SF_C4, SF_C4, SF_C4, SF_C4, SF_C4, SF_C4, SF_C4, SF_C4},      {SF_C1, SF_C3, SF_C5, SF_C7, -SF_C7, -SF_C5, -SF_C3, -SF_C1},
                             {SF_C2, SF_C6, -SF_C6, -SF_C2, -SF_C2, -SF_C6, SF_C6, SF_C2},  {SF_C3, -SF_C7, -SF_C1, -SF_C5, SF_C5, SF_C1, SF_C7, -SF_C3},
                             {SF_C4, -SF_C4, -SF_C4, SF_C4, SF_C4, -SF_C4, -SF_C4, SF_C4},  {SF_C5, -SF_C1, SF_C7, SF_C3, -SF_C3, -SF_C7, SF_C1, -SF_C5},
                             {SF_C6, -SF_C2, SF_C2, -SF_C6, -SF_C6, SF_C2, -SF_C2, SF_C6},  {SF_C7, -SF_C5, SF_C3, -SF_C1, SF_C1, -SF_C3, SF_C5, -SF_C7}};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double s = 0.0;
#pragma unroll
    for (int n = 0; n < 8; ++n) s += D[k][n] * x[n];
    o[k] = s;
  }
}

// the demo's truncation, rounded after the multiply and after the add as torch's two kernels do: contraction is switched
// off here, a fused multiply-add lands on the other side of an integer for ~4e-6 of the values (hipcc contracts
// __fmul_rn / __fadd_rn like plain operators)
__device__ __forceinline__ float to_u8(float p, int range01) {
#pragma clang fp contract(off)
  if (range01) return truncf(255.f * fminf(fmaxf(p, 0.f), 1.f));
  const float scaled = fminf(fmaxf(p, -1.f), 1.f) * 127.5f;
  return truncf(scaled + 127.5f);
}

__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
  const f32x4 t = *(const f32x4*)p;
  v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
}
__device__ __forceinline__ void load4(const bf16_t* p, float (&v)[4]) {
  const bf16x4 t = *(const bf16x4*)p;
  v[0] = bf2f(t.x), v[1] = bf2f(t.y), v[2] = bf2f(t.z), v[3] = bf2f(t.w);
}

// grid (ceil(W / 64), MCU rows, N) x 256 threads.  T = float / bf16_t: planar [N][3][H][W]; T = uint8_t: [N][H][W][3].
template <typename T, bool SUB420>
__global__ __launch_bounds__(256) void jpeg_transform_kernel(const T* __restrict__ frames, int16_t* __restrict__ coef, const QuantTables qt, int H, int W,
                                                             int range01, int mcus_x, int blocks_per_frame) {
  constexpr int ROWS = SUB420 ? 16 : 8, MCU = SUB420 ? 16 : 8, BPM = SUB420 ? 6 : 3, MPT = TILE_W / MCU;
  __shared__ __attribute__((aligned(16))) double sPlane[3][16 * PLANE_LD];
  __shared__ double sT[TILE_BLOCKS * T_BLOCK];
  __shared__ __attribute__((aligned(16))) int16_t sOut[TILE_BLOCKS * 64];
  const int t = threadIdx.x, tile = blockIdx.x, my = blockIdx.y;
  const long n = blockIdx.z;
  const int x0 = tile * TILE_W;
  const int tile_mcus = min(MPT, mcus_x - tile * MPT);

  // 1. four pixels per thread: truncate to 8 bit, JFIF YCbCr (Y level-shifted, chroma without its + 128), stage in LDS
  if (t < ROWS * 16) {
    const int row = t >> 4, x = x0 + (t & 15) * 4;
    if (x < W) {
      const long y = (long)my * ROWS + row;
      float r[4], g[4], b[4];
      if constexpr (sizeof(T) == 1) {
        const uint32_t* p = (const uint32_t*)((const uint8_t*)frames + ((n * H + y) * W + x) * 3);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
        r[0] = (float)(w0 & 255), g[0] = (float)((w0 >> 8) & 255), b[0] = (float)((w0 >> 16) & 255);
        r[1] = (float)(w0 >> 24), g[1] = (float)(w1 & 255), b[1] = (float)((w1 >> 8) & 255);
        r[2] = (float)((w1 >> 16) & 255), g[2] = (float)(w1 >> 24), b[2] = (float)(w2 & 255);
        r[3] = (float)((w2 >> 8) & 255), g[3] = (float)((w2 >> 16) & 255), b[3] = (float)(w2 >> 24);
      } else {
        const long plane = (long)H * W;
        const T* p = frames + (n * 3 * H + y) * W + x;
        load4(p, r);
        load4(p + plane, g);
        load4(p + 2 * plane, b);
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = to_u8(r[i], range01), g[i] = to_u8(g[i], range01), b[i] = to_u8(b[i], range01);
      }
      const int o = row * PLANE_LD + (t & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double R = r[i], G = g[i], B = b[i];
        sPlane[0][o + i] = 0.299 * R + 0.587 * G + 0.114 * B - 128.0;
        sPlane[1][o + i] = -0.168736 * R - 0.331264 * G + 0.5 * B;
        sPlane[2][o + i] = 0.5 * R - 0.418688 * G - 0.081312 * B;
      }
    }
  }
  __syncthreads();

  // 2. rows: thread (block, row) -> 8 values along x
  const int blk = t >> 3, lane8 = t & 7;
  const int m = blk / BPM, k = blk - m * BPM;
  const bool live = t < TILE_BLOCKS * 8 && m < tile_mcus;
  const int comp = SUB420 ? (k < 4 ? 0 : k - 3) : k;
  if (live) {
    double x[8], o[8];
    if (SUB420 && k >= 4) {
      const double* p = &sPlane[comp][2 * lane8 * PLANE_LD + m * 16];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = 0.25 * ((p[2 * j] + p[2 * j + 1]) + (p[PLANE_LD + 2 * j] + p[PLANE_LD + 2 * j + 1]));
    } else {
      const int bx = SUB420 ? m * 16 + (k & 1) * 8 : m * 8, by = SUB420 ? (k >> 1) * 8 : 0;
      const double* p = &sPlane[comp][(by + lane8) * PLANE_LD + bx];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = p[j];
    }
    dct8(x, o);
#pragma unroll
    for (int u = 0; u < 8; ++u) sT[blk * T_BLOCK + lane8 * T_LD + u] = o[u];
  }
  __syncthreads();

  // 3. columns: thread (block, column) -> 8 coefficients, quantised (a true division, ties to even) and zigzagged
  if (live) {
    double x[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = sT[blk * T_BLOCK + i * T_LD + lane8];
    dct8(x, o);
    const int tbl = comp ? 1 : 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int nat = v * 8 + lane8;
      sOut[blk * 64 + qt.izz[nat]] = (int16_t)(int)rint(o[v] / (double)qt.q[tbl][nat]);
    }
  }
  __syncthreads();

  // 4. the tile's blocks are contiguous in the output: 16 bytes per thread
  if (t * 8 < tile_mcus * BPM * 64) {
    int16_t* dst = coef + (n * blocks_per_frame + ((long)my * mcus_x + tile * MPT) * BPM) * 64;
    *(u32x4*)(dst + t * 8) = *(const u32x4*)&sOut[t * 8];
  }
}

// ------------------------------------------------------------------------------------------------ entropy coding
struct BitSink {
  uint32_t* slot;
  uint64_t acc;
  int pending, words, bits;
  __device__ __forceinline__ void put(uint32_t value, int len) {
    acc = (acc << len) | value;
    pending += len;
    bits += len;
    if (pending >= 32) {
      pending -= 32;
      slot[words++] = (uint32_t)(acc >> pending);
    }
  }
  __device__ __forceinline__ void flush() {
    if (pending > 0) slot[words++] = (uint32_t)(acc << (32 - pending));      // left-aligned, zeros behind
  }
};

// category of v and the category's low bits (a negative value is coded as v - 1), T.81 F.1.2.1
__device__ __forceinline__ void magnitude(int v, int max_cat, int& cat, uint32_t& low, int& bad) {
  const int a = v < 0 ? -v : v;
  cat = a == 0 ? 0 : 32 - __builtin_clz(a);
  if (cat > max_cat) cat = max_cat, bad = 1;
  low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
}

// grid (intervals, N) x 64 threads: one wave per restart interval
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ slots, uint32_t* __restrict__ lens,
                                                          int* __restrict__ status, const HuffTables ht, int bpm, int mcus, int ri, int blocks_per_frame,
                                                          unsigned slot_bytes) {
  __shared__ uint32_t sHuff[2 * 16 + 2 * 256];
  __shared__ uint32_t sSlot[64 * SLOT_DW];
  __shared__ uint32_t sMerge[MERGE_DW];
  const int lane = threadIdx.x, iv = blockIdx.x;
  const long f = blockIdx.y;
  for (int i = lane; i < 2 * 16 + 2 * 256; i += 64) sHuff[i] = ht.t[i];
  const int mcu0 = iv * ri;
  const int nblocks = min(ri, mcus - mcu0) * bpm;
  const int16_t* cf = coef + (f * blocks_per_frame + (long)mcu0 * bpm) * 64;
  uint8_t* out = slots + (f * gridDim.x + iv) * (size_t)slot_bytes;
  unsigned gpos = 0;                     // bytes of this interval written so far, stuffing included
  int carry_bits = 0, bad = 0, overflow = 0;
  uint32_t carry_val = 0;
  __syncthreads();

  for (int c0 = 0; c0 < nblocks; c0 += 64) {
    const int j = c0 + lane;
    BitSink sink{&sSlot[lane * SLOT_DW], 0, 0, 0, 0};
    if (j < nblocks) {
      const int k = j % bpm;
      const int comp = bpm == 6 ? (k < 4 ? 0 : k - 3) : k;
      const int prev = bpm == 6 ? (comp ? j - 6 : (k ? j - 1 : j - 3)) : j - 3;   // the component's previous block
      const int pred = prev >= 0 ? (int)cf[(long)prev * 64] : 0;
      const uint32_t* dc = &sHuff[HUFF_DC + (comp ? 16 : 0)];
      const uint32_t* ac = &sHuff[HUFF_AC + (comp ? 256 : 0)];
      u32x4 raw[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) raw[i] = *(const u32x4*)(cf + (long)j * 64 + i * 8);
      auto value = [&](int i) -> int { return (int)(int16_t)(raw[i >> 3][(i >> 1) & 3] >> ((i & 1) * 16)); };
      int cat;
      uint32_t low;
      magnitude(value(0) - pred, 11, cat, low, bad);
      uint32_t e = dc[cat];
      sink.put(((e & 0xFFFFu) << cat) | low, (int)(e >> 16) + cat);
      int run = 0;
#pragma unroll
      for (int i = 1; i < 64; ++i) {
        const int v = value(i);
        if (v == 0) {
          ++run;
        } else {
          for (; run >= 16; run -= 16) sink.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));      // ZRL
          magnitude(v, 10, cat, low, bad);
          e = ac[(run << 4) | cat];
          sink.put(((e & 0xFFFFu) << cat) | low, (int)(e >> 16) + cat);
          run = 0;
        }
      }
      if (run > 0) sink.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));                                // EOB
      sink.flush();
    }

    // where this lane's bits start: the carried bits of the previous chunk, then the lanes below
    int incl = sink.bits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    const int total = carry_bits + __shfl(incl, 63);
    const int off = carry_bits + incl - sink.bits;
    const bool last = c0 + 64 >= nblocks;
    const int pad = last ? (8 - (total & 7)) & 7 : 0;
    const int ndw = (total + pad + 31) / 32 + 1;
    for (int i = lane; i < ndw; i += 64) sMerge[i] = 0;
    __syncthreads();
    if (lane == 0) {
      if (carry_bits) atomicOr(&sMerge[0], carry_val << (32 - carry_bits));
      if (pad) atomicOr(&sMerge[total >> 5], ((1u << pad) - 1u) << (32 - (total & 31) - pad));   // 1-bits up to the byte boundary
    }
    for (int i = 0; i < sink.words; ++i) {
      const uint32_t w = sink.slot[i];
      const int p = off + 32 * i, sh = p & 31;
      atomicOr(&sMerge[p >> 5], w >> sh);
      if (sh) atomicOr(&sMerge[(p >> 5) + 1], w << (32 - sh));
    }
    __syncthreads();

    // whole bytes go out, 0xFF followed by a stuffed 0x00; the bits behind them are carried into the next chunk
    const int nbytes = (total + pad) >> 3;
    unsigned ffs = 0;
    for (int i0 = 0; i0 < nbytes; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < nbytes;
      const uint32_t b = valid ? (sMerge[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu : 0u;
      const bool ff = b == 0xFFu;
      const uint64_t mask = __ballot(ff);
      const unsigned pos = gpos + i + ffs + __popcll(mask & ((1ull << lane) - 1ull));
      if (valid) {
        if (pos + (ff ? 2u : 1u) <= slot_bytes) {
          out[pos] = (uint8_t)b;
          if (ff) out[pos + 1] = 0;
        } else {
          overflow = 1;
        }
      }
      ffs += __popcll(mask);
    }
    gpos += nbytes + ffs;
    carry_bits = (total + pad) & 7;
    carry_val = carry_bits ? ((sMerge[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xFFu) >> (8 - carry_bits) : 0u;
    __syncthreads();
  }
  const bool any_overflow = __ballot(overflow) != 0, any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    lens[f * gridDim.x + iv] = gpos < slot_bytes ? gpos : slot_bytes;
    const int flags = (any_overflow ? SF_JPEG_SLOT_OVERFLOW : 0) | (any_bad ? SF_JPEG_COEF_RANGE : 0);
    if (flags) atomicOr(status, flags);
  }
}

// ------------------------------------------------------------------------------------------------ pack
// grid N x 256: ipos[f][i] = where interval i starts inside frame f's file (each interval is followed by a 2-byte marker)
__global__ __launch_bounds__(256) void jpeg_scan_intervals_kernel(const uint32_t* __restrict__ lens, uint32_t* __restrict__ ipos, uint32_t* __restrict__ fsize,
                                                                  int intervals, int hdr_len) {
  __shared__ uint32_t s[256];
  const int t = threadIdx.x;
  const long f = blockIdx.x;
  uint32_t running = (uint32_t)hdr_len;
  for (int base = 0; base < intervals; base += 256) {
    const int i = base + t;
    const uint32_t v = i < intervals ? lens[f * intervals + i] + 2u : 0u;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const uint32_t x = t >= o ? s[t - o] : 0u;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    if (i < intervals) ipos[f * intervals + i] = running + s[t] - v;
    running += s[255];
    __syncthreads();
  }
  if (t == 0) fsize[f] = running;
}

// one workgroup: offsets[f] = sum of the file sizes in front of frame f; offsets[n] = all bytes
__global__ __launch_bounds__(256) void jpeg_scan_frames_kernel(const uint32_t* __restrict__ fsize, int64_t* __restrict__ offsets, int n, int64_t capacity,
                                                               int* __restrict__ status) {
  __shared__ int64_t s[256];
  const int t = threadIdx.x;
  int64_t running = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    const int64_t v = i < n ? (int64_t)fsize[i] : 0;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int64_t x = t >= o ? s[t - o] : 0;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    if (i < n) offsets[i] = running + s[t] - v;
    running += s[255];
    __syncthreads();
  }
  if (t == 0) {
    offsets[n] = running;
    if (running > capacity) atomicOr(status, SF_JPEG_OUT_OVERFLOW);
  }
}

// grid (intervals, N) x 256: one interval each; interval 0 also writes the header.  Nothing is written when the files do
// not fit `capacity` (the same test jpeg_scan_frames_kernel turned into a status flag).
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ lens, const uint32_t* __restrict__ ipos,
                                                        const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, const JpegHeader hd, unsigned slot_bytes,
                                                        int64_t capacity) {
  const int t = threadIdx.x, iv = blockIdx.x, intervals = gridDim.x;
  const long f = blockIdx.y;
  if (offsets[gridDim.y] > capacity) return;
  uint8_t* file = out + offsets[f];
  if (iv == 0)
    for (int i = t; i < hd.len; i += 256) file[i] = hd.b[i];
  const long slot = f * intervals + iv;
  const uint8_t* src = slots + slot * (size_t)slot_bytes;
  const unsigned len = lens[slot];
  uint8_t* dst = file + ipos[slot];
  for (unsigned i = t; i < len; i += 256) dst[i] = src[i];
  if (t == 0) {
    dst[len] = 0xFF;
    dst[len + 1] = (uint8_t)(iv == intervals - 1 ? 0xD9 : 0xD0 + (iv & 7));     // EOI behind the last interval, RSTn between
  }
}

int check_common(const char* who, int quality) {
  SF_CHECK(quality >= 1 && quality <= 100, "%s: quality=%d (1..100)", who, quality);
  return 0;
}

}  // namespace

extern "C" size_t sf_jpeg_workspace_bytes(int n, int h, int w, int subsampling, int restart_interval) {
  Geometry g;
  if (geometry("sf_jpeg_workspace_bytes", n, h, w, subsampling, restart_interval, &g) != 0) return 0;
  return g.total;
}

extern "C" int sf_jpeg_transform(const void* frames, int dtype, int value_range, int n, int h, int w, int subsampling, int quality, void* coef,
                                 void* stream) {
  const char* who = "sf_jpeg_transform";
  Geometry g;
  SF_TRY(geometry(who, n, h, w, subsampling, 1, &g));
  SF_TRY(check_common(who, quality));
  SF_CHECK(frames && coef, "%s: null buffer", who);
  SF_CHECK(dtype >= SF_JPEG_U8 && dtype <= SF_JPEG_BF16, "%s: unknown dtype %d", who, dtype);
  SF_CHECK(value_range == SF_JPEG_RANGE_PM1 || value_range == SF_JPEG_RANGE_01, "%s: unknown value range %d", who, value_range);
  SF_CHECK((uintptr_t)frames % 16 == 0 && (uintptr_t)coef % 16 == 0, "%s: buffers must be 16-byte aligned", who);
  QuantTables qt;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) qt.q[t][i] = (float)quant_value(kBaseQuant[t][i], quality);
  for (int k = 0; k < 64; ++k) qt.izz[kZigzag[k]] = (uint8_t)k;
  const dim3 grid((unsigned)((w + TILE_W - 1) / TILE_W), (unsigned)g.mcus_y, (unsigned)n), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int r01 = value_range == SF_JPEG_RANGE_01;
  const auto launch = [&](auto sub420) {
    return pixel_dispatch(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      return sf_launch<&jpeg_transform_kernel<T, decltype(sub420)::value>>(who, grid, block, 0, s, (const T*)frames, (int16_t*)coef, qt, h, w, r01, g.mcus_x, g.blocks);
    });
  };
  return subsampling == SF_JPEG_420 ? launch(std::true_type{}) : launch(std::false_type{});
}

extern "C" int sf_jpeg_entropy(const void* coef, int n, int h, int w, int subsampling, int quality, int restart_interval, void* workspace,
                               size_t workspace_bytes, void* out, size_t out_capacity, int64_t* offsets, int32_t* status, void* stream) {
  const char* who = "sf_jpeg_entropy";
  Geometry g;
  SF_TRY(geometry(who, n, h, w, subsampling, restart_interval, &g));
  SF_TRY(check_common(who, quality));
  SF_CHECK(coef && workspace && out && offsets && status, "%s: null buffer", who);
  SF_CHECK((uintptr_t)coef % 16 == 0 && (uintptr_t)workspace % 256 == 0 && (uintptr_t)offsets % 8 == 0 && (uintptr_t)status % 4 == 0,
           "%s: coef must be 16-byte, workspace 256-byte, offsets 8-byte, status 4-byte aligned", who);
  SF_CHECK(workspace_bytes >= g.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g.total);
  SF_CHECK(g.slot_bytes < 0xFFFFFF00u, "%s: a restart interval of %d blocks needs a slot of 4 GiB or more", who, g.interval_blocks);
  JpegHeader hd;
  build_header(h, w, quality, subsampling, restart_interval, &hd);
  SF_CHECK(out_capacity >= (size_t)n * (hd.len + 2), "%s: out_capacity of %zu bytes cannot hold %d headers", who, out_capacity, n);
  static const HuffTables ht = [] {
    HuffTables tmp = {};
    for (int t = 0; t < 2; ++t) {
      huffman_table(kDcBits[t], kDcVals, &tmp.t[HUFF_DC + 16 * t]);
      huffman_table(kAcBits[t], kAcVals[t], &tmp.t[HUFF_AC + 256 * t]);
    }
    return tmp;
  }();
  char* ws = (char*)workspace;
  uint8_t* slots = (uint8_t*)(ws + g.slots_off);
  uint32_t* lens = (uint32_t*)(ws + g.lens_off);
  uint32_t* ipos = (uint32_t*)(ws + g.ipos_off);
  uint32_t* fsize = (uint32_t*)(ws + g.fsize_off);
  hipStream_t s = (hipStream_t)stream;
  SF_TRY(sf_hip_ok(hipMemsetAsync(status, 0, 4, s), who, "clearing the status word"));
  const dim3 per_interval((unsigned)g.intervals, (unsigned)n);
  SF_TRY(sf_launch<&jpeg_entropy_kernel>(who, per_interval, dim3(64), 0, s, (const int16_t*)coef, slots, lens, (int*)status, ht, g.bpm, g.mcus,
                                         restart_interval, g.blocks, (unsigned)g.slot_bytes));
  SF_TRY(sf_launch<&jpeg_scan_intervals_kernel>(who, dim3((unsigned)n), dim3(256), 0, s, lens, ipos, fsize, g.intervals, (int)hd.len));
  SF_TRY(sf_launch<&jpeg_scan_frames_kernel>(who, dim3(1), dim3(256), 0, s, fsize, offsets, n, (int64_t)out_capacity, (int*)status));
  return sf_launch<&jpeg_pack_kernel>(who, per_interval, dim3(256), 0, s, slots, lens, ipos, offsets, (uint8_t*)out, hd, (unsigned)g.slot_bytes,
                                      (int64_t)out_capacity);
}

extern "C" int sf_jpeg_encode_frames(const void* frames, int dtype, int value_range, int n, int h, int w, int subsampling, int quality,
                                     int restart_interval, void* workspace, size_t workspace_bytes, void* out, size_t out_capacity, int64_t* offsets,
                                     int32_t* status, void* stream) {
  const char* who = "sf_jpeg_encode_frames";
  Geometry g;
  SF_TRY(geometry(who, n, h, w, subsampling, restart_interval, &g));
  SF_CHECK(workspace && (uintptr_t)workspace % 256 == 0, "%s: workspace must be 256-byte aligned", who);
  SF_CHECK(workspace_bytes >= g.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, g.total);
  SF_CHECK(out && offsets && status, "%s: null buffer", who);
  SF_TRY(sf_jpeg_transform(frames, dtype, value_range, n, h, w, subsampling, quality, workspace, stream));
  return sf_jpeg_entropy(workspace, n, h, w, subsampling, quality, restart_interval, workspace, workspace_bytes, out, out_capacity, offsets, status, stream);
}
