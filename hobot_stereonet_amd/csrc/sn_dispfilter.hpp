// sn_dispfilter.hpp — speckle removal and hole filling of int32 disparity maps (sn_filter_raw; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/dispfilter.py).  All per-pixel arithmetic is integer.
//
// Speckle removal is connected-component labelling under the predicate "both > 0 and |a - b| <= dq" (4-neighbours, the
// difference in 64 bits).  Four kernels, label[] and size[] are the 8 bytes of scratch per pixel:
//   k_flt_label   one workgroup per 64 x 16 tile.  A wave owns four tile rows, lane = column, so the horizontal links of a row
//                 are one __ballot and every pixel's first label is the start of its row run (a bit scan, no memory).  Vertical
//                 links are united in LDS with the lock-free atomicMin union (parent <= index, labels only decrease); a link
//                 whose left neighbour carries the same union (both rows run on, the neighbour is linked upwards too) is
//                 skipped.  Members are counted in LDS, one add per row run; the kernel writes label[p] = the tile root as a
//                 pixel index of the map and size[p] = the member count at a tile root, 0 at every other pixel.
//                 12 bytes per pixel (4 read, 8 written).
//   k_flt_seam    one thread per pixel pair across a tile border; a linked pair unites the two tile roots in global memory with
//                 the same union.  Workgroups on different XCDs meet in label[] inside one launch: the XCDs' L2s are not
//                 coherent and a CU's L1 is never refreshed, so EVERY access to label[] in this kernel is a relaxed agent-scope
//                 atomic (load, fetch_min), never a plain load.  Within one border segment of a tile pair a linked pair whose
//                 predecessor along the border is linked as well, with both along-border links present, is implied by that
//                 predecessor and skipped: a smooth surface costs one union per tile border, not 64.  (The rule stops at
//                 tile corners: across a corner two skipped pairs could each rely on the other.)
//   k_flt_flatten one thread per pixel, only tile roots (size != 0) work: find the final root R, point label[p] at it, add the
//                 tile's count to size[R] — one integer atomic per tile-local component, order-free.  The root of a component
//                 is its smallest pixel index, so labels are deterministic too.  After it root(p) = label[label[p]].
//                 4 bytes per pixel read.
//   k_flt_apply   one wave per row, 64 columns per step, lane = column.  Stage-1 value m = size[root] <= max ? 0 : raw.  The
//                 nearest valid column to the left / right inside the step comes from __ballot + a bit scan and its value from
//                 a shuffle; the carry from the left is a wave-uniform pair, the one from the right a look-ahead that reads
//                 on until it meets a valid pixel and is kept until the walk passes it, so every step is evaluated at most
//                 twice (the second read hits L1 / L2) for any W.  A step is written after its last read and the steps ahead
//                 are still unwritten, so out_raw == raw is safe.  VEC (W % 4 == 0, mask 4-byte aligned): four mask bytes per
//                 dword store.  counts: per-thread integers, one atomicAdd per workgroup and counter.
//                 <= 17 bytes per pixel of first-touch traffic (raw 4, label 4, out 4, mask 1, disp 4) + the root gathers.
// With speckle_max_px == 0 only k_flt_apply runs, without label[] / size[].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_pointcloud.hpp"   // pc_block_sum
#include "../../include/stereonet_hip.h"   // SN_FLT_*

namespace sn {

constexpr int kFltTW = 64, kFltTH = 16, kFltTile = kFltTW * kFltTH;
constexpr int kFltSlice = 8;      // maps per pass over the scratch (8 bytes per pixel and map)

struct FltArgs {
  const int32_t* raw;    // [n][H][W]
  int32_t* out_raw;      // nullable; may be `raw`
  float* disp;           // nullable
  uint8_t* mask;         // nullable
  uint32_t* counts;      // nullable: [n][3], zeroed before the launch
  uint32_t* label;       // [n][H][W] scratch, nullptr without speckle removal
  uint32_t* size;        // [n][H][W] scratch
  int W, H, tiles_x, tiles_y;
  long long dq;          // link threshold in raw units
  uint32_t max_px;       // 0: no speckle removal
  int fill_max;          // 0: no filling
  float S;
};

__device__ __forceinline__ bool flt_linked(int32_t a, int32_t b, long long dq) {
  const long long d = (long long)a - (long long)b;
  return a > 0 && b > 0 && (d < 0 ? -d : d) <= dq;
}

// ---- union-find in LDS (one tile) ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t flt_lds_find(uint32_t* lab, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void flt_lds_union(uint32_t* lab, uint32_t a, uint32_t b) {
  for (;;) {
    a = flt_lds_find(lab, a);
    b = flt_lds_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(lab + a, b);      // a > b: the smaller index wins
    if (old == a) return;
    a = old;                                         // somebody moved a meanwhile: unite its new parent with b
  }
}

// grid (tiles_x * tiles_y, maps)
__global__ __launch_bounds__(256) void k_flt_label(FltArgs a) {
  __shared__ int32_t sraw[kFltTile];
  __shared__ uint32_t lab[kFltTile], cnt[kFltTile];
  __shared__ unsigned long long shl[kFltTH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const size_t map = (size_t)blockIdx.y * a.H * a.W;
  const int32_t* raw = a.raw + map;
  const int u = tx * kFltTW + lane;
  int32_t v[4];
  unsigned long long hb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = wave * 4 + e, y = ty * kFltTH + r;
    v[e] = (u < a.W && y < a.H) ? raw[(size_t)y * a.W + u] : 0;
    sraw[r * kFltTW + lane] = v[e];
    cnt[r * kFltTW + lane] = 0;
    const int32_t left = __shfl_up(v[e], 1);
    hb[e] = __ballot(lane > 0 && flt_linked(left, v[e], a.dq));       // bit l: column l runs on from column l - 1
    if (lane == 0) shl[r] = hb[e];
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
    lab[r * kFltTW + lane] = r * kFltTW + 63 - __builtin_clzll(~hb[e] & upto);      // bit 0 of ~hb is always set
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = wave * 4 + e;
    const int32_t above = e > 0 ? v[e - 1] : (r > 0 ? sraw[(r - 1) * kFltTW + lane] : 0);
    const bool vl = flt_linked(above, v[e], a.dq);
    const unsigned long long vb = __ballot(vl);
    const unsigned long long hba = e > 0 ? hb[e - 1] : (r > 0 ? shl[r - 1] : 0ull);
    const bool implied = lane > 0 && ((hb[e] >> lane) & 1) && ((hba >> lane) & 1) && ((vb >> (lane - 1)) & 1);
    if (vl && !implied) flt_lds_union(lab, r * kFltTW + lane, (r - 1) * kFltTW + lane);
  }
  __syncthreads();
  uint32_t root[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t idx = (wave * 4 + e) * kFltTW + lane;
    uint32_t x = idx;
    while (lab[x] != x) x = lab[x];
    root[e] = x;
    if (v[e] > 0 && !((hb[e] >> lane) & 1)) {      // the start of a row run adds the whole run
      const int len = lane == 63 ? 1 : 1 + __builtin_ctzll(~(hb[e] >> (lane + 1)));
      atomicAdd(cnt + x, (uint32_t)len);
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = wave * 4 + e, y = ty * kFltTH + r;
    if (u >= a.W || y >= a.H) continue;
    const uint32_t idx = r * kFltTW + lane, p = (uint32_t)y * a.W + u;
    const uint32_t rp = (uint32_t)(ty * kFltTH + (root[e] >> 6)) * a.W + tx * kFltTW + (root[e] & 63);
    const bool valid = v[e] > 0;
    a.label[map + p] = valid ? rp : p;
    a.size[map + p] = valid && root[e] == idx ? cnt[idx] : 0u;
  }
}

// ---- union-find in global memory (tile roots of one map), agent-scope atomics only -----------------------------------------
__device__ __forceinline__ uint32_t flt_find(uint32_t* L, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void flt_union(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = flt_find(L, a);
    b = flt_find(L, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// grid (ceil(pairs / 256), maps); pairs = (tiles_x - 1) * H across vertical borders + (tiles_y - 1) * W across horizontal ones
__global__ __launch_bounds__(256) void k_flt_seam(FltArgs a) {
  const int nvs = (a.tiles_x - 1) * a.H, nhs = (a.tiles_y - 1) * a.W;
  int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= nvs + nhs) return;
  const size_t map = (size_t)blockIdx.y * a.H * a.W;
  const int32_t* raw = a.raw + map;
  uint32_t* L = a.label + map;
  uint32_t p1, p2, back;      // the pair, and the step to its predecessor along the border (0: first of its segment)
  if (g < nvs) {
    const int s = g / a.H, y = g - s * a.H;
    p1 = (uint32_t)y * a.W + (s + 1) * kFltTW - 1;
    p2 = p1 + 1;
    back = y % kFltTH ? (uint32_t)a.W : 0u;
  } else {
    g -= nvs;
    const int s = g / a.W, x = g - s * a.W;
    p1 = (uint32_t)((s + 1) * kFltTH - 1) * a.W + x;
    p2 = p1 + a.W;
    back = x % kFltTW ? 1u : 0u;
  }
  const int32_t r1 = raw[p1], r2 = raw[p2];
  if (!flt_linked(r1, r2, a.dq)) return;
  if (back) {
    const int32_t q1 = raw[p1 - back], q2 = raw[p2 - back];
    if (flt_linked(q1, q2, a.dq) && flt_linked(q1, r1, a.dq) && flt_linked(q2, r2, a.dq)) return;
  }
  flt_union(L, p1, p2);      // find walks from the pixels through their tile roots
}

// grid (ceil(H * W / 256), maps)
__global__ __launch_bounds__(256) void k_flt_flatten(FltArgs a) {
  const uint32_t hw = (uint32_t)a.H * a.W, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const size_t map = (size_t)blockIdx.y * hw;
  const uint32_t s = a.size[map + p];      // != 0: p is a tile root; nobody adds to it unless it is a final root
  if (!s) return;
  const uint32_t R = flt_find(a.label + map, p);
  if (R == p) return;
  __hip_atomic_store(a.label + map + p, R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(a.size + map + R, s);
}

// the stage-1 value of column u of a row (0 where the pixel ends stage 1 invalid) and its mask bits
__device__ __forceinline__ int32_t flt_stage1(const FltArgs& a, const int32_t* raw, const uint32_t* label, const uint32_t* size,
                                              size_t row, int u, uint32_t* bits) {
  *bits = 0;
  if (u >= a.W) return 0;
  const int32_t r = raw[row + u];
  if (r <= 0) {
    *bits = SN_FLT_INVALID_IN;
    return 0;
  }
  if (a.max_px && size[label[label[row + u]]] <= a.max_px) {
    *bits = SN_FLT_SPECKLE;
    return 0;
  }
  return r;
}

// grid (workgroups per map, maps); each wave takes whole rows of map blockIdx.y
template <bool VEC>
__global__ __launch_bounds__(256) void k_flt_apply(FltArgs a) {
  __shared__ uint32_t red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t map = (size_t)blockIdx.y * a.H * a.W;
  const int32_t* raw = a.raw + map;
  const uint32_t* label = a.max_px ? a.label + map : nullptr;
  const uint32_t* size = a.max_px ? a.size + map : nullptr;
  const int steps = (a.W + 63) >> 6;
  const unsigned long long below_me = (1ull << lane) - 1, above_me = lane == 63 ? 0ull : ~((2ull << lane) - 1);
  uint32_t n_valid = 0, n_speckle = 0, n_filled = 0;
  for (int v = blockIdx.x * 4 + wave; v < a.H; v += gridDim.x * 4) {
    const size_t row = (size_t)v * a.W;
    int lcol = -1, rcol = -1;        // nearest valid column before this step (-1: none); first valid column at or after
    int32_t lval = 0, rval = 0;      // `ahead` (W: none), valid while rcol >= the end of the step
    for (int c = 0; c < steps; ++c) {
      const int base = c << 6, u = base + lane;
      uint32_t bits;
      const int32_t m = flt_stage1(a, raw, label, size, row, u, &bits);
      const unsigned long long bal = __ballot(m > 0);
      if (a.fill_max && rcol < base + 64) {      // the look-ahead is stale: read on until a valid pixel or the end of the row
        rcol = a.W;
        for (int c2 = c + 1; c2 < steps; ++c2) {
          uint32_t b2;
          const int32_t m2 = flt_stage1(a, raw, label, size, row, (c2 << 6) + lane, &b2);
          const unsigned long long bal2 = __ballot(m2 > 0);
          if (bal2) {
            const int src = __builtin_ctzll(bal2);
            rcol = (c2 << 6) + src;
            rval = __shfl(m2, src);
            break;
          }
        }
      }
      int32_t out = m;
      if (a.fill_max) {
        const unsigned long long lo = bal & below_me, hi = bal & above_me;
        const int sl = lo ? 63 - __builtin_clzll(lo) : 0, sr = hi ? __builtin_ctzll(hi) : 0;
        const int32_t ml = __shfl(m, sl), mr = __shfl(m, sr);
        const int ul = lo ? base + sl : lcol, ur = hi ? base + sr : rcol;
        const int32_t vl = lo ? ml : lval, vr = hi ? mr : rval;
        if (m <= 0 && u < a.W && (ul >= 0 || ur < a.W) && ur - ul - 1 <= a.fill_max) {
          out = ul < 0 ? vr : (ur >= a.W ? vl : min(vl, vr));
          bits |= SN_FLT_FILLED;
        }
        if (bal) {
          const int last = 63 - __builtin_clzll(bal);
          lcol = base + last;
          lval = __shfl(m, last);
        }
      }
      n_valid += out > 0;
      n_speckle += (bits & SN_FLT_SPECKLE) != 0;
      n_filled += (bits & SN_FLT_FILLED) != 0;
      if (a.mask) {
        if (VEC) {
          const uint32_t w = bits | (__shfl_down(bits, 1) << 8) | (__shfl_down(bits, 2) << 16) | (__shfl_down(bits, 3) << 24);
          if (!(lane & 3) && u < a.W) *reinterpret_cast<uint32_t*>(a.mask + map + row + u) = w;
        } else if (u < a.W) {
          a.mask[map + row + u] = (uint8_t)bits;
        }
      }
      if (u < a.W) {
        if (a.out_raw) a.out_raw[map + row + u] = out;
        if (a.disp && bits) a.disp[map + row + u] = out > 0 ? (float)out * a.S : 0.f;
      }
    }
  }
  if (a.counts) {
    const uint32_t t0 = pc_block_sum(n_valid, red), t1 = pc_block_sum(n_speckle, red), t2 = pc_block_sum(n_filled, red);
    if (threadIdx.x == 0) {
      if (t0) atomicAdd(a.counts + blockIdx.y * 3 + 0, t0);
      if (t1) atomicAdd(a.counts + blockIdx.y * 3 + 1, t1);
      if (t2) atomicAdd(a.counts + blockIdx.y * 3 + 2, t2);
    }
  }
}

}  // namespace sn
