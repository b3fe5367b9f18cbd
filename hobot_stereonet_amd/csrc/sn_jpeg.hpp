// sn_jpeg.hpp — baseline JPEG of NV12 images on the GPU (sn_jpeg_encode_nv12; the contract is in include/stereonet_hip.h, the
// numpy twin is hobot_stereonet_amd/jpeg.py, the authority is the host encoder csrc/compat/src/jpeg_nv12.cpp, whose bytes
// these kernels reproduce).  Part of the single translation unit stereonet_hip.hip.
//
// A stream is header, slice 0, RST0, slice 1, RST1, ..., last slice, EOI.  A slice is a restart interval of rows_per_slice MCU
// rows: byte aligned, DC predictors reset, so slices are independent and the parallelism is frames x slices.  A single-scan
// stream (rows_per_slice = 0) is ONE sequential chain per frame: one workgroup walks the whole frame.  It is correct, not
// fast; use rows_per_slice = 1 where the consumer accepts restart markers.
//
// Three kernels, not fused: the coefficients make a round trip through the lane's scratch (128 bytes per block).
//   k_jpeg_dct       one thread per 8x8 block, the block in registers: samples (edge-replicated) -> AAN forward DCT in fp32
//                    in the host's order of operations (vertical pass, transpose, vertical pass) under
//                    `#pragma clang fp contract(off)` -> multiply by the reciprocal quantiser, round to nearest even ->
//                    zigzagged int16 [frame][mcu][6][64].  Optionally the fp32 coefficients before quantisation.
//   k_jpeg_entropy   one workgroup of kJpgT threads per (slice, frame), the slice in chunks of kJpgT blocks, one block per
//                    thread: code length of the block (its own coefficients + the previous same-component DC) -> prefix sum
//                    = bit offsets -> the codes ORed into a big-endian bit buffer in LDS (32-bit LDS atomics) -> byte
//                    stuffing by a second prefix sum over the 0xFF bytes -> the lane's scratch; the partial last byte is
//                    carried into the next chunk, the last chunk pads with ones.  A block takes at most 20 + 63 * 26 bits
//                    (208 bytes), 416 stuffed.
//   k_jpeg_assemble  one workgroup per (slice, frame): the slice lengths of the frame summed -> offset and total; the
//                    capacity check BEFORE any byte is stored (sizes[k] = 0 and nothing written if the stream does not fit);
//                    header (built on the host, in the kernel arguments), slice bytes, marker.
#pragma once

namespace sn {

constexpr int kJpgSlice = 8;              // frames per pass over the scratch
constexpr int kJpgT = 128;                // threads of k_jpeg_entropy = blocks per chunk
constexpr int kJpgBlockBytes = 208;       // unstuffed bound of one block: 20 + 63 * 26 = 1658 bits
constexpr int kJpgBufWords = kJpgT * kJpgBlockBytes / 4 + 4;
constexpr int kJpgHuffWords = 16 + 16 + 256 + 256;      // DC luma, DC chroma, AC luma, AC chroma; entry = code << 5 | length
constexpr int kJpgHeaderMax = 632;        // 623 + 6 with DRI

struct JpgDctArgs {
  const uint8_t* nv12;
  int16_t* coef;          // [frame][blocks][64], zigzag order
  float* dct;             // nullable: [frame][blocks][64] fp32 before quantisation, coefficient (v, u) at u * 8 + v
  size_t frame;           // bytes between frames
  int pitch, w, h, mw, blocks;      // blocks = MCUs * 6 of one frame
  float rl[64], rc[64];   // reciprocal quantisers, zigzag order
};

struct JpgEntArgs {
  const int16_t* coef;
  uint8_t* bytes;         // [frame][slice][cap_slice] stuffed entropy-coded bytes
  uint32_t* lens;         // [frame][slice]
  size_t cap_slice;
  int blocks, blocks_per_slice, nslices;
  uint32_t huff[kJpgHuffWords];
};

struct JpgAsmArgs {
  const uint8_t* bytes;
  const uint32_t* lens;
  uint8_t* out;
  uint32_t* sizes;
  size_t out_stride, cap_slice;
  int nslices, hdr_len;
  uint8_t hdr[kJpgHeaderMax];
};

// One AAN 8-point DCT along the first (ALONG == 0) or second index of d, for all 8 positions of the other index: aan_pass of
// the host encoder, operation by operation.
template <int ALONG>
__device__ __forceinline__ void jpg_aan_pass(float (&d)[8][8]) {
#pragma clang fp contract(off)
#define JPG_D(i) (ALONG == 0 ? d[i][c] : d[c][i])
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float t0 = JPG_D(0) + JPG_D(7), t7 = JPG_D(0) - JPG_D(7);
    const float t1 = JPG_D(1) + JPG_D(6), t6 = JPG_D(1) - JPG_D(6);
    const float t2 = JPG_D(2) + JPG_D(5), t5 = JPG_D(2) - JPG_D(5);
    const float t3 = JPG_D(3) + JPG_D(4), t4 = JPG_D(3) - JPG_D(4);
    const float e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    JPG_D(0) = e0 + e1;
    JPG_D(4) = e0 - e1;
    const float z1 = (e2 + e3) * 0.707106781f;
    JPG_D(2) = e3 + z1;
    JPG_D(6) = e3 - z1;
    const float o0 = t4 + t5, o1 = t5 + t6, o2 = t6 + t7;
    const float z5 = (o0 - o2) * 0.382683433f;
    const float z2 = 0.541196100f * o0 + z5;
    const float z4 = 1.306562965f * o2 + z5;
    const float z3 = o1 * 0.707106781f;
    const float z11 = t7 + z3, z13 = t7 - z3;
    JPG_D(5) = z13 + z2;
    JPG_D(3) = z13 - z2;
    JPG_D(1) = z11 + z4;
    JPG_D(7) = z11 - z4;
  }
#undef JPG_D
}

// grid (ceil(blocks / 256), frames)
__global__ __launch_bounds__(256) void k_jpeg_dct(JpgDctArgs a) {
#pragma clang fp contract(off)
  static constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  const int blk = blockIdx.x * 256 + threadIdx.x;
  if (blk >= a.blocks) return;
  const int mcu = blk / 6, j = blk - mcu * 6, my = mcu / a.mw, mx = mcu - my * a.mw;
  const uint8_t* img = a.nv12 + blockIdx.y * a.frame;
  const bool luma = j < 4;
  const uint8_t* plane = luma ? img : img + (size_t)a.h * a.pitch + (j - 4);
  const int step = luma ? 1 : 2, pw = luma ? a.w : a.w >> 1, ph = luma ? a.h : a.h >> 1;
  const int bx = luma ? mx * 16 + (j & 1) * 8 : mx * 8, by = luma ? my * 16 + (j >> 1) * 8 : my * 8;
  float d[8][8];
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint8_t* row = plane + (size_t)min(by + y, ph - 1) * a.pitch;
#pragma unroll
    for (int x = 0; x < 8; ++x) d[y][x] = (float)row[min(bx + x, pw - 1) * step] - 128.0f;
  }
  jpg_aan_pass<0>(d);      // vertical
  jpg_aan_pass<1>(d);      // horizontal: the host's second vertical pass on the transposed block
  const size_t at = ((size_t)blockIdx.y * a.blocks + blk) * 64;
  if (a.dct) {             // the host's layout after the transpose: coefficient (v, u) at u * 8 + v
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int v = 0; v < 8; ++v) a.dct[at + u * 8 + v] = d[v][u];
  }
  const float* recip = luma ? a.rl : a.rc;
  uint32_t packed[32];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int v = kZigzag[i] >> 3, u = kZigzag[i] & 7;
    const int q = (int)rintf(d[v][u] * recip[i]);
    if (i & 1) packed[i >> 1] |= (uint32_t)q << 16;
    else packed[i >> 1] = (uint32_t)q & 0xffffu;
  }
  uint4* dst = reinterpret_cast<uint4*>(a.coef + at);
#pragma unroll
  for (int g = 0; g < 8; ++g) dst[g] = make_uint4(packed[4 * g], packed[4 * g + 1], packed[4 * g + 2], packed[4 * g + 3]);
}

// `len` bits (1..31; 0: nothing) of `code` (< 2^len) at bit `pos` of the big-endian bit buffer
__device__ __forceinline__ void jpg_put(uint32_t* buf, uint32_t pos, uint32_t code, int len) {
  if (!len) return;
  const uint64_t v = (uint64_t)code << (64 - (int)(pos & 31) - len);
  atomicOr(&buf[pos >> 5], (uint32_t)(v >> 32));
  const uint32_t lo = (uint32_t)v;
  if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}

__device__ __forceinline__ int jpg_category(int v) { return 32 - __clz(v < 0 ? -v : v); }
__device__ __forceinline__ uint32_t jpg_magnitude(int v, int nb) { return (uint32_t)(v < 0 ? v + (1 << nb) - 1 : v) & ((1u << nb) - 1); }

// The code of one block: DC difference, AC run / size symbols with ZRL for runs over 15, EOB unless coefficient 63 is non-zero.
// Returns its length in bits; EMIT: also ORs it into buf from bit `pos` on.
template <bool EMIT>
__device__ __forceinline__ uint32_t jpg_block_code(const int16_t* __restrict__ c, int pred, const uint32_t* dc, const uint32_t* ac,
                                                   uint32_t* buf, uint32_t pos) {
  const uint32_t start = pos;
  const uint4* q = reinterpret_cast<const uint4*>(c);
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const uint4 w4 = q[g];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int v = (int)(int16_t)(w[e >> 1] >> ((e & 1) * 16));
      if (g == 0 && e == 0) {
        const int diff = v - pred, nb = jpg_category(diff);
        const uint32_t t = dc[min(nb, 15)];
        if (EMIT) {
          jpg_put(buf, pos, t >> 5, t & 31);
          jpg_put(buf, pos + (t & 31), jpg_magnitude(diff, nb), nb);
        }
        pos += (t & 31) + nb;
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        const uint32_t z = ac[0xF0];
        if (EMIT) jpg_put(buf, pos, z >> 5, z & 31);
        pos += z & 31;
        run -= 16;
      }
      const int nb = jpg_category(v);
      const uint32_t t = ac[(run << 4) | min(nb, 15)];
      if (EMIT) jpg_put(buf, pos, ((t >> 5) << nb) | jpg_magnitude(v, nb), (int)(t & 31) + nb);
      pos += (t & 31) + nb;
      run = 0;
    }
  }
  if (run) {
    const uint32_t t = ac[0];
    if (EMIT) jpg_put(buf, pos, t >> 5, t & 31);
    pos += t & 31;
  }
  return pos - start;
}

// inclusive prefix sum of one value per thread over the kJpgT threads; *all = the sum.  wsum: kJpgT / 64 words
__device__ __forceinline__ uint32_t jpg_scan(uint32_t v, uint32_t* wsum, uint32_t* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  __syncthreads();      // the previous use of wsum is over
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  uint32_t before = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < kJpgT / 64; ++i) {
    if (i < wave) before += wsum[i];
    sum += wsum[i];
  }
  *all = sum;
  return v + before;
}

// grid (slices, frames)
__global__ __launch_bounds__(kJpgT) void k_jpeg_entropy(JpgEntArgs a) {
  __shared__ uint32_t buf[kJpgBufWords];
  __shared__ uint32_t huff[kJpgHuffWords];
  __shared__ uint32_t wsum[kJpgT / 64];
  const int t = threadIdx.x, s = blockIdx.x, k = blockIdx.y;
  const int first = s * a.blocks_per_slice, count = min(a.blocks_per_slice, a.blocks - first);
  const int16_t* coef = a.coef + ((size_t)k * a.blocks + first) * 64;
  uint8_t* dst = a.bytes + ((size_t)k * a.nslices + s) * a.cap_slice;
  for (int i = t; i < kJpgHuffWords; i += kJpgT) huff[i] = a.huff[i];
  uint32_t rem = 0, carry = 0;      // the partial byte the previous chunk left: its bits (0..7) and the byte
  uint32_t outpos = 0;              // stuffed bytes written so far
  for (int b0 = 0; b0 < count; b0 += kJpgT) {
    __syncthreads();                // the previous chunk's bytes are read (first chunk: the tables are there)
    for (int i = t; i < kJpgBufWords; i += kJpgT) buf[i] = 0;
    __syncthreads();
    if (t == 0) buf[0] = carry << 24;
    const int b = b0 + t;
    const bool live = b < count;
    const int j = b % 6;            // `first` is a whole number of MCUs
    const bool luma = j < 4;
    // the previous block of the same component within the slice: Y follows the block before it, or Y3 of the MCU before
    const int pb = (j >= 1 && j <= 3) ? b - 1 : (b >= 6 ? (j == 0 ? b - 3 : b - 6) : -1);
    const int pred = live && pb >= 0 ? (int)coef[(size_t)pb * 64] : 0;
    const uint32_t* dc = huff + (luma ? 0 : 16);
    const uint32_t* ac = huff + (luma ? 32 : 288);
    const int16_t* c = coef + (size_t)b * 64;
    const uint32_t len = live ? jpg_block_code<false>(c, pred, dc, ac, buf, 0) : 0;
    uint32_t total;
    const uint32_t incl = jpg_scan(len, wsum, &total);      // its barriers also order buf[0] before the ORs
    if (live) jpg_block_code<true>(c, pred, dc, ac, buf, rem + incl - len);
    __syncthreads();
    const bool last = b0 + kJpgT >= count;
    const uint32_t bits = rem + total;
    uint32_t nb = bits >> 3;        // whole bytes of this chunk
    rem = bits & 7;
    if (last && rem) {              // the slice ends: pad the last partial byte with ones
      if (t == 0) buf[nb >> 2] |= ((1u << (8 - rem)) - 1) << (24 - 8 * (nb & 3));
      ++nb;
      rem = 0;
      __syncthreads();
    }
    for (uint32_t base = 0; base < nb; base += kJpgT * 4) {      // stuffing: four bytes per thread and round
      const uint32_t idx = base + t * 4;
      const int valid = idx < nb ? (int)min(4u, nb - idx) : 0;
      const uint32_t word = valid ? buf[idx >> 2] : 0;
      uint32_t ffs = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) ffs += (e < valid && ((word >> (24 - 8 * e)) & 0xFF) == 0xFF) ? 1 : 0;
      uint32_t round_ffs;
      const uint32_t incl_ff = jpg_scan(ffs, wsum, &round_ffs);
      uint8_t* p = dst + outpos + t * 4 + (incl_ff - ffs);      // outpos: everything before this round
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < valid) {
          const uint8_t byte = (uint8_t)(word >> (24 - 8 * e));
          *p++ = byte;
          if (byte == 0xFF) *p++ = 0;
        }
      outpos += min((uint32_t)kJpgT * 4, nb - base) + round_ffs;
    }
    carry = (buf[nb >> 2] >> (24 - 8 * (nb & 3))) & 0xFF;      // rem == 0: unused
  }
  if (t == 0) a.lens[(size_t)k * a.nslices + s] = outpos;
}

// grid (slices, frames)
__global__ __launch_bounds__(256) void k_jpeg_assemble(JpgAsmArgs a) {
  __shared__ uint32_t red[4];
  const int t = threadIdx.x, s = blockIdx.x, k = blockIdx.y;
  const uint32_t* lens = a.lens + (size_t)k * a.nslices;
  uint32_t before = 0, total = 0;
  for (int i = t; i < a.nslices; i += 256) {
    const uint32_t l = lens[i];
    total += l;
    if (i < s) before += l;
  }
  before = pc_block_sum(before, red);
  total = pc_block_sum(total, red);
  const size_t all = (size_t)a.hdr_len + total + 2 * (size_t)a.nslices;
  const bool fits = all <= a.out_stride;
  if (s == 0 && t == 0) a.sizes[k] = fits ? (uint32_t)all : 0u;
  if (!fits) return;      // nothing of this frame is stored
  uint8_t* o = a.out + (size_t)k * a.out_stride;
  if (s == 0)
    for (int i = t; i < a.hdr_len; i += 256) o[i] = a.hdr[i];
  uint8_t* d = o + a.hdr_len + before + 2 * (size_t)s;
  const uint8_t* src = a.bytes + ((size_t)k * a.nslices + s) * a.cap_slice;
  const uint32_t len = lens[s];
  for (uint32_t i = t; i < len; i += 256) d[i] = src[i];
  if (t == 0) {
    d[len] = 0xFF;
    d[len + 1] = s + 1 < a.nslices ? (uint8_t)(0xD0 + (s & 7)) : (uint8_t)0xD9;
  }
}

// ---- host side: tables and header (jpeg_nv12.cpp's make_tables / JpegAppendHeader) ---------------------------------------------
const uint8_t kJpgZigzagHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kJpgQLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                              14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                              18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kJpgQChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kJpgDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kJpgDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kJpgDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kJpgAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kJpgAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kJpgAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kJpgAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

inline int jpg_clamp_quality(int q) { return q < 1 ? 1 : (q > 100 ? 100 : q); }
inline int jpg_mcu_rows(int h) { return (h + 15) / 16; }
// MCUs per restart interval; 0: a single scan without DRI
inline long long jpg_restart_mcus(int w, int h, int rows_per_slice) {
  return rows_per_slice <= 0 || rows_per_slice >= jpg_mcu_rows(h) ? 0 : (long long)rows_per_slice * ((w + 15) / 16);
}
inline bool jpg_size_ok(int w, int h) { return w >= 2 && h >= 2 && w <= 65535 && h <= 65535 && !(w & 1) && !(h & 1); }

// A capacity no stream of a w x h image can exceed: header, 416 stuffed bytes per block, a marker and a pad byte per MCU row
inline size_t jpg_bound(int w, int h) {
  if (!jpg_size_ok(w, h)) return 0;
  const size_t mw = (size_t)(w + 15) / 16, rows = (size_t)jpg_mcu_rows(h);
  return 640 + mw * rows * 6 * (2 * kJpgBlockBytes) + rows * 4;
}

// What a call needs besides the image, built once per (w, h, quality, restart interval) and kept on the lane
struct JpgPlan {
  int w = 0, h = 0, quality = 0, restart = -1;
  uint8_t ql[64], qc[64];      // natural order
  float rl[64], rc[64];        // zigzag order
  uint32_t huff[kJpgHuffWords];
  uint8_t hdr[kJpgHeaderMax];
  int hdr_len = 0;
};

inline void jpg_huff(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i) table[vals[k++]] = ((uint32_t)code++ << 5) | (uint32_t)l;
    code <<= 1;
  }
}

inline void jpg_make_plan(int w, int h, int quality, int restart, JpgPlan* p) {
  static const double aan[8] = {1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379};
  quality = jpg_clamp_quality(quality);
  if (p->w == w && p->h == h && p->quality == quality && p->restart == restart) return;
  const int sf = quality < 50 ? 5000 / quality : 200 - quality * 2;
  for (int i = 0; i < 64; ++i) {
    const int a = (kJpgQLum[i] * sf + 50) / 100, b = (kJpgQChr[i] * sf + 50) / 100;
    p->ql[i] = (uint8_t)(a < 1 ? 1 : (a > 255 ? 255 : a));
    p->qc[i] = (uint8_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
  }
  for (int i = 0; i < 64; ++i) {
    const int nat = kJpgZigzagHost[i], v = nat >> 3, u = nat & 7;
    const double s = aan[u] * aan[v] * 8.0;
    p->rl[i] = (float)(1.0 / (p->ql[nat] * s));
    p->rc[i] = (float)(1.0 / (p->qc[nat] * s));
  }
  memset(p->huff, 0, sizeof p->huff);
  jpg_huff(kJpgDcLumBits, kJpgDcVals, p->huff);
  jpg_huff(kJpgDcChrBits, kJpgDcVals, p->huff + 16);
  jpg_huff(kJpgAcLumBits, kJpgAcLumVals, p->huff + 32);
  jpg_huff(kJpgAcChrBits, kJpgAcChrVals, p->huff + 288);
  uint8_t* o = p->hdr;
  auto put = [&](std::initializer_list<int> v) { for (int b : v) *o++ = (uint8_t)b; };
  auto copy = [&](const uint8_t* src, int n) { memcpy(o, src, n), o += n; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int i = 0; i < 64; ++i) *o++ = (t ? p->qc : p->ql)[kJpgZigzagHost[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  auto dht = [&](int cls, const uint8_t* bits, const uint8_t* vals, int nvals) {
    put({0xFF, 0xC4, (19 + nvals) >> 8, (19 + nvals) & 255, cls});
    copy(bits, 16);
    copy(vals, nvals);
  };
  dht(0x00, kJpgDcLumBits, kJpgDcVals, 12);
  dht(0x10, kJpgAcLumBits, kJpgAcLumVals, 162);
  dht(0x01, kJpgDcChrBits, kJpgDcVals, 12);
  dht(0x11, kJpgAcChrBits, kJpgAcChrVals, 162);
  if (restart > 0) put({0xFF, 0xDD, 0, 4, restart >> 8, restart & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  p->hdr_len = (int)(o - p->hdr);
  p->w = w, p->h = h, p->quality = quality, p->restart = restart;
}

}  // namespace sn
