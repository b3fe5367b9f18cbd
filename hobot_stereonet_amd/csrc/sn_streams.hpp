// sn_streams.hpp — the device side of the stream and torus layer under k_temporal, k_costmap and k_el_fuse (the group lists and
// their host side are in sn_stream_groups.hpp).  Every helper is forced inline: the kernels compile to what they were with
// the code written out.
//
//   torus         a window of mw x mh cells rolls with the pose: world cell (cx, cy) lives in slot (cx mod mw, cy mod mh), and
//                 slot (i, j) under origin (ox, oy) holds world cell (ox + (i - ox) mod mw, oy + (j - oy) mod mh).
//   stats_*       per-frame statistics of four counters: a lane's counters of a frame are packed into two words of 16-bit
//                 fields, summed over the wave by shuffles and added to an LDS table [frame][4] by one lane per wave; after the
//                 last frame one global atomicAdd per workgroup, frame and non-zero counter (integer, order-free).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_stream_groups.hpp"

namespace sn {

__host__ __device__ __forceinline__ int torus_mod(int a, int m) {      // floor modulo, m > 0
  const int r = a % m;
  return r < 0 ? r + m : r;
}

// (i - o) mod m for 0 <= i < m, with om = o mod m: no division per lane
__device__ __forceinline__ int torus_unroll(int i, int om, int m) {
  const int u = i - om;
  return u < 0 ? u + m : u;
}

// the world cell that slot i of a row or column of m slots holds under origin o
__device__ __forceinline__ int torus_cell(int i, int o, int m) { return o + torus_unroll(i, torus_mod(o, m), m); }

// The roll test: under the previous origin (pox, poy) slot (i, j) held another world cell than (cx, cy), so `forget` it.  It
// takes the action, not a bool to its caller: a predicate that returns one compiles k_costmap and k_el_fuse to other registers
// than the test written out in place does (profiles/stream_layer_codegen.md)
template <class F>
__device__ __forceinline__ void torus_if_rolled(bool seen, int i, int j, int cx, int cy, int pox, int poy, int mw, int mh, F forget) {
  if (seen && (cx != torus_cell(i, pox, mw) || cy != torus_cell(j, poy, mh))) forget();
}

// before the first frame (a barrier follows): the table of the group's frames starts at zero
__device__ __forceinline__ void stats_clear(uint32_t (*cnt)[4], int frames) {
  if ((int)threadIdx.x < frames * 4) cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;
}

// one frame, the whole wave: lo and hi hold two counters each, and a wave's sums stay below 2^16
__device__ __forceinline__ void stats_frame(uint32_t* c, uint32_t lo, uint32_t hi) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    lo += __shfl_xor(lo, s);
    hi += __shfl_xor(hi, s);
  }
  if ((threadIdx.x & 63) == 0) {
    if (lo & 0xffffu) atomicAdd(c + 0, lo & 0xffffu);
    if (lo >> 16) atomicAdd(c + 1, lo >> 16);
    if (hi & 0xffffu) atomicAdd(c + 2, hi & 0xffffu);
    if (hi >> 16) atomicAdd(c + 3, hi >> 16);
  }
}

// after the last frame, the whole workgroup: out[map[f]][4] += cnt[f - f0] for the group's frames f0 .. f1 - 1
__device__ __forceinline__ void stats_flush(const uint32_t (*cnt)[4], uint32_t* out, const int* map, int f0, int f1) {
  __syncthreads();
  if ((int)threadIdx.x < (f1 - f0) * 4) {
    const uint32_t v = cnt[threadIdx.x >> 2][threadIdx.x & 3];
    if (v) atomicAdd(out + (size_t)map[f0 + (threadIdx.x >> 2)] * 4 + (threadIdx.x & 3), v);
  }
}

}  // namespace sn
