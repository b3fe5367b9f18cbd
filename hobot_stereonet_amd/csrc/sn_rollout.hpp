// sn_rollout.hpp — the trajectory rollout: from the inflated grid, the navigation function and the robot's pose to the best
// velocity sample and its trajectory (sn_rollout; the contract is in include/stereonet_hip.h, the numpy twin is
// hobot_stereonet_amd/rollout.py).  All trigonometry is in the two host tables built here (ro_tables); the kernels are integer.
//
//   k_rollout_eval  grid (nw * ceil(nv / 4), maps), 256 threads: a WAVE per sample, a workgroup the four samples iv..iv+3 of one
//                   iw, so that the four share that iw's offset rows, which the workgroup first copies into LDS ((T+1) * nf
//                   pairs, dynamic, sized by the call).  A lane per (step, point) pair, t-major, 64 pairs a pass: the centre's
//                   row of `centres` (a broadcast within the lanes of one step), the offset from LDS, the rotation by the pose
//                   in int64, one byte gathered from the cost grid.  The first colliding step is a min over the lanes and occ a
//                   max; because the pairs are t-major, a pass in which any lane collided ends the walk: no later pass holds a
//                   smaller step.  Lane 0 reads the potential under the last centre and stores the sample's two words.
//                   One map has S waves: a few hundred to a thousand at batch 1, which covers the part, where a lane per
//                   sample would fill a handful of CUs.
//   k_rollout_best  grid (maps), 256 threads: re-reads the samples' words (the call keeps them in a buffer of its own where the
//                   caller wants none), counts the four reasons, takes the minimum of score << 16 | s over the valid ones
//                   (an integer minimum: any order gives the same word), writes best and the winner's trajectory.
// No atomics, nothing zeroed beforehand, nothing persistent, no workgroup waits for another; every store is a plain vector store.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stereonet_hip.h"

namespace sn {

constexpr int kRoWaves = 4;                     // samples (waves) of a workgroup of k_rollout_eval
constexpr int kRoThreads = 64 * kRoWaves;
constexpr int kRoBestThreads = 256;
constexpr int kRoMaxSide = 4096;                // gw, gh (their product: SN_NAV_MAX_CELLS, the potential is sn_navfn's)
constexpr int kRoNoHit = 0x7fffffff;
constexpr double kRoTwoPi = 6.283185307179586;
constexpr double kRoMaxTheta = 1048576.0;       // fabs(th), fabs(yaw)
constexpr long long kRoMaxReach = 1 << 21;      // |centre + offset| per component, in 1/256 cell

// nullptr, or why sn_rollout_tables refuses the parameters and the footprint (the tables' own range test is ro_tables')
inline const char* ro_params_check(const sn_rollout_params* p, const float* footprint, int nf) {
  if (!p) return "a NULL pointer";
  for (float v : {p->cell_m, p->v_min, p->v_max, p->w_min, p->w_max, p->sim_time_s})
    if (!std::isfinite(v)) return "every parameter must be finite";
  if (!(p->cell_m > 0.f)) return "cell_m must be positive";
  if (!(p->sim_time_s > 0.f)) return "sim_time_s must be positive";
  if (p->v_max < p->v_min || p->w_max < p->w_min) return "v_min <= v_max and w_min <= w_max are required";
  if (p->nv < 1 || p->nv > SN_ROLLOUT_MAX_SIDE || p->nw < 1 || p->nw > SN_ROLLOUT_MAX_SIDE) return "nv and nw must be 1..64";
  if (p->steps < 1 || p->steps > SN_ROLLOUT_MAX_STEPS) return "steps must be 1..64";
  if (p->lethal_cost < 1 || p->lethal_cost > 255) return "lethal_cost must be 1..255";
  if (p->centre_lethal_cost < 1 || p->centre_lethal_cost > 255) return "centre_lethal_cost must be 1..255";
  if (p->unknown_cost < 0 || p->unknown_cost > 252) return "unknown_cost must be 0..252";
  if (p->flags & ~SN_ROLLOUT_UNKNOWN_OK) return "flags has bits other than SN_ROLLOUT_UNKNOWN_OK";
  if (p->w_goal < 0 || p->w_goal > 32767 || p->w_occ < 0 || p->w_occ > 32767) return "w_goal and w_occ must be 0..32767";
  if (p->w_goal == 0 && p->w_occ == 0) return "w_goal and w_occ must not both be 0";
  if (nf < 0 || nf > SN_ROLLOUT_MAX_POINTS) return "nf must be 0..64";
  if (nf > 0 && !footprint) return "a NULL footprint";
  for (int i = 0; i < 2 * nf; ++i)
    if (!std::isfinite(footprint[i])) return "the footprint must be finite";
  return nullptr;
}

// v(i) or w(i) of the lattice
inline double ro_lattice(float lo, float hi, int count, int i) {
#pragma clang fp contract(off)
  if (count == 1) return (double)lo;
  const double step = ((double)hi - (double)lo) / (double)(count - 1);
  return (double)lo + (double)i * step;
}

// The contract's tables for parameters ro_params_check accepts; either output may be null.  nullptr, or why they are refused.
inline const char* ro_tables(const sn_rollout_params* p, const float* footprint, int nf, int32_t* centres, int32_t* offsets) {
#pragma clang fp contract(off)
  const int T = p->steps, nv = p->nv, nw = p->nw;
  const double k256 = 256.0 / (double)p->cell_m;
  const double lim = (double)kRoMaxReach;
  for (int iw = 0; iw < nw; ++iw) {
    const double w = ro_lattice(p->w_min, p->w_max, nw, iw);
    for (int t = 0; t <= T; ++t) {
      const double tau = ((double)p->sim_time_s * (double)t) / (double)T;
      const double th = w * tau;
      if (!(fabs(th) <= kRoMaxTheta)) return "the heading turns by more than 2^20 rad";
      const double c = cos(th), s = sin(th);
      // the offsets of this (iw, t), and their extent: the largest |centre| they may be added to
      double ox[SN_ROLLOUT_MAX_POINTS], oy[SN_ROLLOUT_MAX_POINTS];
      for (int f = 0; f < nf; ++f) {
        const double fx = (double)footprint[2 * f], fy = (double)footprint[2 * f + 1];
        ox[f] = (c * fx - s * fy) * k256, oy[f] = (s * fx + c * fy) * k256;
        if (!(fabs(ox[f]) <= lim) || !(fabs(oy[f]) <= lim)) return "a footprint point lies more than 2^21 / 256 cells from the centre";
        if (offsets) {
          int32_t* o = offsets + (((size_t)iw * (T + 1) + t) * nf + f) * 2;
          o[0] = (int32_t)llrint(ox[f]), o[1] = (int32_t)llrint(oy[f]);
        }
      }
      const long long bam = llrint((th / kRoTwoPi) * 65536.0) & 0xFFFF;
      for (int iv = 0; iv < nv; ++iv) {
        const double v = ro_lattice(p->v_min, p->v_max, nv, iv);
        double x, y;
        if (fabs(th) < 1e-6) {
          x = v * tau;
          y = ((v * tau) * th) / 2.0;
        } else {
          const double r = v / w;
          x = r * s;
          y = r * (1.0 - c);
        }
        const double xs = x * k256, ys = y * k256;
        if (!(fabs(xs) <= lim) || !(fabs(ys) <= lim)) return "an arc reaches more than 2^21 / 256 cells from its start";
        const long long cx = llrint(xs), cy = llrint(ys);
        for (int f = 0; f < nf; ++f) {
          const long long qx = cx + llrint(ox[f]), qy = cy + llrint(oy[f]);
          if (qx > kRoMaxReach || qx < -kRoMaxReach || qy > kRoMaxReach || qy < -kRoMaxReach)
            return "a footprint point reaches more than 2^21 / 256 cells from the arc's start";
        }
        if (centres) {
          int32_t* o = centres + (((size_t)iv * nw + iw) * (T + 1) + t) * 3;
          o[0] = (int32_t)cx, o[1] = (int32_t)cy, o[2] = (int32_t)bam;
        }
      }
    }
  }
  return nullptr;
}

// the contract's q of a pose; false where sn_rollout_pose_q refuses it
inline bool ro_pose_q(float cell_m, double ox, double oy, const double* pose, int32_t* q) {
#pragma clang fp contract(off)
  if (!std::isfinite(cell_m) || !(cell_m > 0.f) || !std::isfinite(ox) || !std::isfinite(oy)) return false;
  const double x = pose[0], y = pose[1], yaw = pose[2], lim = 1073741824.0;
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(yaw) || !(fabs(yaw) <= kRoMaxTheta)) return false;
  const double k256 = 256.0 / (double)cell_m;
  const double fx = (x - ox) * k256, fy = (y - oy) * k256;
  if (!(fabs(fx) <= lim) || !(fabs(fy) <= lim)) return false;
  q[0] = (int32_t)llrint(fx), q[1] = (int32_t)llrint(fy);
  q[2] = (int32_t)llrint(cos(yaw) * lim), q[3] = (int32_t)llrint(sin(yaw) * lim);
  q[4] = (int32_t)(llrint((yaw / kRoTwoPi) * 65536.0) & 0xFFFF);
  return true;
}

struct RoArgs {
  const uint8_t* cost;        // [maps][gh][gw]
  const uint32_t* pot;        // [maps][gh][gw]
  const int32_t* poses;       // [maps][5]
  const int32_t* window;      // nullable: [maps][4]
  const int32_t* centres;     // [S][T+1][3]
  const int32_t* offsets;     // [nw][T+1][nf][2], 8-byte aligned
  uint32_t* samples;          // [maps][S][2]
  uint32_t* best;             // nullable: [maps][8]
  int32_t* traj;              // nullable: [maps][T+1][3]
  int gw, gh, nv, nw, T, nf;
  int lethal, centre_lethal, unknown_cost, flags, w_goal, w_occ;
};

// a point {qx, qy} of the robot's frame in grid sub-units: the contract's X and Y
struct RoPose {
  long long px, py, cq, sq;
  __device__ __forceinline__ long long X(int qx, int qy) const { return px + ((cq * qx - sq * qy + (1ll << 29)) >> 30); }
  __device__ __forceinline__ long long Y(int qx, int qy) const { return py + ((sq * qx + cq * qy + (1ll << 29)) >> 30); }
};

__device__ __forceinline__ RoPose ro_pose(const int32_t* q) { return RoPose{q[0], q[1], q[2], q[3]}; }

__global__ __launch_bounds__(kRoThreads) void k_rollout_eval(RoArgs a) {
  extern __shared__ int2 s_off[];      // [T+1][nf]: the offset rows of this workgroup's iw
  const int map = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int iw = blockIdx.x % a.nw, iv = (blockIdx.x / a.nw) * kRoWaves + (tid >> 6);
  const int steps1 = a.T + 1, pts = a.nf + 1, S = a.nv * a.nw;
  int iv_lo = 0, iv_hi = a.nv - 1, iw_lo = 0, iw_hi = a.nw - 1;
  if (a.window) {
    const int32_t* win = a.window + 4 * map;
    iv_lo = win[0], iv_hi = win[1], iw_lo = win[2], iw_hi = win[3];
  }
  const bool iw_in = iw >= iw_lo && iw <= iw_hi;      // the same for the whole workgroup
  if (iw_in) {
    const int2* rows = reinterpret_cast<const int2*>(a.offsets) + (size_t)iw * steps1 * a.nf;
    for (int i = tid; i < steps1 * a.nf; i += kRoThreads) s_off[i] = rows[i];
  }
  __syncthreads();
  if (iv >= a.nv) return;
  const int s = iv * a.nw + iw;
  uint32_t* out = a.samples + ((size_t)map * S + s) * 2;
  if (!iw_in || iv < iv_lo || iv > iv_hi) {
    if (lane == 0) out[0] = SN_NAV_INF, out[1] = (uint32_t)SN_ROLLOUT_OUT_OF_WINDOW << 8;
    return;
  }
  const RoPose pose = ro_pose(a.poses + 5 * map);
  const int32_t* cen = a.centres + (size_t)s * steps1 * 3;
  const size_t cells = (size_t)a.gw * a.gh;
  const uint8_t* cost = a.cost + map * cells;
  const int items = steps1 * pts;
  int hit = kRoNoHit, occ = 0;
  for (int base = 0; base < items; base += 64) {
    const int i = base + lane;
    if (i < items) {
      const int t = i / pts, f = i - t * pts;      // f == 0: the centre
      int qx = cen[3 * t], qy = cen[3 * t + 1];
      if (f) {
        const int2 o = s_off[t * a.nf + f - 1];
        qx += o.x, qy += o.y;
      }
      const long long cx = pose.X(qx, qy) >> 8, cy = pose.Y(qx, qy) >> 8;
      int price = -1;      // collides
      if (cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh) {
        const int c = cost[(size_t)cy * a.gw + (size_t)cx];
        if (c == 255) price = (a.flags & SN_ROLLOUT_UNKNOWN_OK) ? a.unknown_cost : -1;
        else if (c < (f ? a.lethal : a.centre_lethal)) price = c;
      }
      if (price < 0) hit = min(hit, t);
      else occ = max(occ, price);
    }
    if (__any(hit != kRoNoHit)) break;      // t-major: every later pair has a step at least as large
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    hit = min(hit, __shfl_xor(hit, off));
    occ = max(occ, __shfl_xor(occ, off));
  }
  if (lane != 0) return;
  if (hit != kRoNoHit) {
    out[0] = SN_NAV_INF, out[1] = (uint32_t)SN_ROLLOUT_COLLISION << 8 | (uint32_t)hit << 16;
    return;
  }
  // the last centre did not collide, so its cell lies inside the grid
  const int qx = cen[3 * a.T], qy = cen[3 * a.T + 1];
  const long long cx = pose.X(qx, qy) >> 8, cy = pose.Y(qx, qy) >> 8;
  const uint32_t g = a.pot[map * cells + (size_t)cy * a.gw + (size_t)cx];
  out[0] = g, out[1] = g == SN_NAV_INF ? (uint32_t)SN_ROLLOUT_NO_ROUTE << 8 : (uint32_t)occ;
}

__global__ __launch_bounds__(kRoBestThreads) void k_rollout_best(RoArgs a) {
  __shared__ unsigned long long s_key[kRoBestThreads / 64];
  __shared__ uint32_t s_count[kRoBestThreads / 64][4];
  __shared__ unsigned long long s_best;
  const int map = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.nv * a.nw, steps1 = a.T + 1;
  const uint32_t* samples = a.samples + (size_t)map * S * 2;
  unsigned long long key = ~0ull;
  uint32_t count[4] = {0, 0, 0, 0};
  for (int s = tid; s < S; s += kRoBestThreads) {
    const uint2 w{samples[2 * s], samples[2 * s + 1]};      // the caller's buffer is only 4-byte aligned
    const uint32_t reason = w.y >> 8 & 0xffu;
#pragma unroll
    for (int r = 0; r < 4; ++r) count[r] += reason == (uint32_t)r;
    if (reason == SN_ROLLOUT_VALID) {
      const unsigned long long score = (unsigned long long)a.w_goal * w.x + (unsigned long long)a.w_occ * (w.y & 0xffu);
      const unsigned long long k = score << 16 | (unsigned)s;
      key = k < key ? k : key;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off);
    key = other < key ? other : key;
#pragma unroll
    for (int r = 0; r < 4; ++r) count[r] += __shfl_xor(count[r], off);
  }
  if (lane == 0) {
    s_key[wave] = key;
#pragma unroll
    for (int r = 0; r < 4; ++r) s_count[wave][r] = count[r];
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t total[4] = {0, 0, 0, 0};
    for (int w = 0; w < kRoBestThreads / 64; ++w) {
      key = s_key[w] < key ? s_key[w] : key;
      for (int r = 0; r < 4; ++r) total[r] += s_count[w][r];
    }
    s_best = key;
    if (a.best) {
      uint32_t* best = a.best + (size_t)map * 8;
      const bool none = key == ~0ull;
      const unsigned long long score = key >> 16;
      best[0] = none ? (uint32_t)SN_ROLLOUT_NO_VALID : 0u;
      best[1] = none ? 0xFFFFFFFFu : (uint32_t)(key & 0xFFFFu);
      best[2] = none ? 0xFFFFFFFFu : (uint32_t)score;
      best[3] = none ? 0xFFFFFFFFu : (uint32_t)(score >> 32);
      best[4] = total[SN_ROLLOUT_VALID], best[5] = total[SN_ROLLOUT_COLLISION], best[6] = total[SN_ROLLOUT_NO_ROUTE];
      best[7] = total[SN_ROLLOUT_OUT_OF_WINDOW];
    }
  }
  __syncthreads();
  if (!a.traj || s_best == ~0ull) return;
  const int sb = (int)(s_best & 0xFFFFu);
  const int32_t* q = a.poses + 5 * map;
  const RoPose pose = ro_pose(q);
  const int32_t* cen = a.centres + (size_t)sb * steps1 * 3;
  int32_t* traj = a.traj + (size_t)map * steps1 * 3;
  for (int t = tid; t < steps1; t += kRoBestThreads) {
    const int qx = cen[3 * t], qy = cen[3 * t + 1];
    traj[3 * t] = (int32_t)pose.X(qx, qy), traj[3 * t + 1] = (int32_t)pose.Y(qx, qy);
    traj[3 * t + 2] = (q[4] + cen[3 * t + 2]) & 0xFFFF;
  }
}

}  // namespace sn
