// sn_ground.hpp — int32 disparity map -> the dominant ground plane of a region, the mount it implies and a per-pixel label
// (sn_ground_from_raw, include/stereonet_hip.h).  A plane in space is a plane in (u, v, raw), so every decision is taken on
// integers and equals the numpy twin's (hobot_stereonet_amd/ground.py) byte for byte; the two places that work in double (the
// refit's 2x2 solve, the geometry) run in one lane each with a fixed order of + - * / sqrt and no FMA.
//   k_gr_fill      one launch starts every accumulator (the hypotheses' counts, usable, the moments of every round) at 0.
//   k_gr_hyp       a lane per hypothesis and map: three samples -> the integer cross product (A, B, C, D), C > 0, or dead
//                  (an unusable sample, |C| < min_area, outside the gate: rationals against integer bounds by cross-multiplying).
//   k_gr_score     the hot path.  A workgroup stages a tile of up to kGrRows sample rows x 256 columns in LDS (0 = unusable).  Lanes own
//                  hypotheses (A, B, C, D in registers), read the samples as LDS broadcasts and count in a register: along a row
//                  A*u + B*v - D is a running 64-bit add and C*r one 32 x 32 -> 64 multiply-add.  With K <= 128 the 256 lanes
//                  are 256 / K' groups that share the tile's rows (K' = 64 or 128).  One integer atomicAdd per lane and tile.
//   k_gr_select    a workgroup per map: the highest count, ties to the lowest index; one lane quantises the winner to Q16.
//   k_gr_moments   the nine int64 moments over the inliers of the current Q16 plane: block sums, nine atomics per workgroup.
//   k_gr_solve     a lane per map: the centred normal equations in double -> the next Q16 plane, or singular: keep and stop.
//   k_gr_finish    a lane per map: flags, the gate on the final plane, height / normal / mount in double -> the sn_ground record.
//   k_gr_labels    every pixel of the map against the final plane: memory-bound, 16-byte loads where the map allows them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/stereonet_hip.h"
#include "sn_pointcloud.hpp"      // pc_block_sum

namespace sn {

constexpr int kGrMaxHyp = 1024, kGrMaxRefits = 4;
constexpr int kGrRows = 8;                                   // sample rows of a tile, at most
constexpr int kGrWorkgroups = 512;                           // a call has at least this many tiles, or tiles of the fewest rows
constexpr int32_t kGrMaxRaw = 1 << 24;                       // a usable sample: 0 < r <= kGrMaxRaw
constexpr int64_t kGrSlopeLim = (int64_t)1 << 34;            // |a|, |b| in Q16 (gate and refit)
constexpr int64_t kGrOffsetLim = (int64_t)1 << 41;           // |c| in Q16

struct GrHyp {
  int64_t A, B, D;
  int32_t C, pad;      // C > 0, or 0: dead
};

struct GrState {
  int64_t q[3];        // the current plane in Q16: a, b, c at (u0, v0)
  int32_t has;         // a hypothesis survived
  int32_t stop;        // a refit was singular: the plane stays
  int32_t winner;
  uint32_t survivors;
};

// The region's sample grid: samples (j0 + sj, i0 + si), sj < Ws, si < Hs, at (u, v) = (j * step, i * step); centre (u0, v0).
struct GrRoi {
  int j0, i0, Ws, Hs, u0, v0;
};

struct GrArgs {
  const int32_t* raw;      // [n][H][W]
  int W, H, step, n;
  GrRoi roi;
  int rows;                // sample rows of a tile of k_gr_score: 1, 2, 4 or 8 (gr_rows)
  int K, min_area, min_inliers, refits;
  uint32_t seed;
  int64_t tol;             // tol_raw
  int64_t gate[6];
  GrHyp* hyp;              // [n][K]
  uint32_t* counts;        // [n][K]
  unsigned long long* acc; // [n][acc_words]: usable, then nine moments per round
  int acc_words;
  GrState* state;          // [n]
  sn_ground* out;          // [n]
  uint8_t* labels;         // [n][H][W], nullable
  float m[12];             // the prior mount, resolved
  float fx, fy, cx, cy, baseline_mm, S;
};

// nullptr and *r, or why the region is refused
inline const char* gr_roi(const sn_ground_params* p, int W, int H, int step, GrRoi* r) {
  int x = p->roi_x, y = p->roi_y, w = p->roi_w, h = p->roi_h;
  if (!x && !y && !w && !h) y = H / 2, w = W, h = H - H / 2;      // the lower half at full width
  if (x < 0 || y < 0 || w < 1 || h < 1 || x > W - w || y > H - h) return "the region of interest must lie inside the image";
  r->j0 = (x + step - 1) / step, r->i0 = (y + step - 1) / step;
  r->Ws = (x + w + step - 1) / step - r->j0, r->Hs = (y + h + step - 1) / step - r->i0;
  r->u0 = x + w / 2, r->v0 = y + h / 2;
  if (r->Ws < 1 || r->Hs < 1 || (int64_t)r->Ws * r->Hs < 3) return "the region of interest must hold at least three samples";
  return nullptr;
}

// The rows of a tile: kGrRows where the call has tiles enough to fill the device, else halved down to the number of lane groups
// that share a tile's rows in k_gr_score (a single map is otherwise a few dozen workgroups of long serial loops).
inline int gr_rows(const GrRoi& roi, int K, int n) {
  const int parts = K <= 64 ? 4 : (K <= 128 ? 2 : 1), tiles_x = (roi.Ws + 255) / 256;
  int rows = kGrRows;
  while (rows > parts && (int64_t)tiles_x * ((roi.Hs + rows - 1) / rows) * n < kGrWorkgroups) rows >>= 1;
  return rows;
}

inline float gr_scale(float out_scale) { return (float)((double)out_scale * 192.0); }

// the prior mount: all twelve zero = the level forward mount
inline void gr_prior(const sn_ground_params* p, float* m) {
  bool level = true;
  for (float v : p->base_from_cam) level = level && v == 0.f;
  const float level_mount[12] = {0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0};
  for (int i = 0; i < 12; ++i) m[i] = level ? level_mount[i] : p->base_from_cam[i];
}

// sn_ground_gate: the header states the arithmetic.  double, a fixed order; cos and sin are the host's.
inline void gr_gate(const sn_camera* cam, const sn_ground_params* p, const GrRoi& roi, float out_scale, int64_t* gate) {
  float m[12];
  gr_prior(p, m);
  const double S = (double)gr_scale(out_scale), Bm = (double)cam->baseline_mm / 1000.0, fx = cam->fx, fy = cam->fy;
  const double x0[3] = {m[0], m[1], m[2]}, y0[3] = {m[4], m[5], m[6]}, n0[3] = {-(double)m[8], -(double)m[9], -(double)m[10]};
  const double tilt[3] = {0.0, -(double)p->max_tilt_rad, (double)p->max_tilt_rad};
  const double height[2] = {(double)p->height_min_m, (double)p->height_max_m};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int ia = 0; ia < 3; ++ia)
    for (int ib = 0; ib < 3; ++ib)
      for (int ih = 0; ih < 2; ++ih) {
        const double ca = std::cos(tilt[ia]), sa = std::sin(tilt[ia]), cb = std::cos(tilt[ib]), sb = std::sin(tilt[ib]);
        double nn[3];
        for (int e = 0; e < 3; ++e) nn[e] = cb * (ca * n0[e] + sa * y0[e]) + sb * x0[e];
        const double g = Bm / (height[ih] * S);
        const double a = g * nn[0], b = g * nn[1] * fx / fy, cp = g * nn[2] * fx;
        const double c = (cp + a * ((double)roi.u0 - (double)cam->cx)) + b * ((double)roi.v0 - (double)cam->cy);
        const double q[3] = {a * 65536.0, b * 65536.0, c * 65536.0};
        for (int e = 0; e < 3; ++e) lo[e] = q[e] < lo[e] ? q[e] : lo[e], hi[e] = q[e] > hi[e] ? q[e] : hi[e];
      }
  for (int e = 0; e < 3; ++e) {
    const double lim = (double)(e < 2 ? kGrSlopeLim : kGrOffsetLim);
    const double l = std::floor(lo[e]), h = std::ceil(hi[e]);
    gate[2 * e] = (int64_t)(l < -lim ? -lim : (l > lim ? lim : l));
    gate[2 * e + 1] = (int64_t)(h < -lim ? -lim : (h > lim ? lim : h));
  }
}

__host__ __device__ __forceinline__ uint32_t gr_mix(uint32_t seed, uint32_t i) {
  uint32_t x = seed + i * 0x9E3779B9u;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ bool gr_usable(int32_t r) { return r > 0 && r <= kGrMaxRaw; }

__device__ __forceinline__ int64_t gr_abs(int64_t v) { return v < 0 ? -v : v; }

// (int64)floor(x * 65536 + 0.5) where |x * 65536| <= lim, else false
__device__ __forceinline__ bool gr_q16(double x, int64_t lim, int64_t* q) {
#pragma clang fp contract(off)
  const double s = x * 65536.0;
  if (!(s >= -(double)lim && s <= (double)lim)) return false;      // NaN included
  *q = (int64_t)floor(s + 0.5);
  return true;
}

struct GrFillArgs {
  uint32_t* counts;
  unsigned long long* acc;
  size_t n_counts, n_acc;
};

__global__ __launch_bounds__(256) void k_gr_fill(GrFillArgs a) {
  const size_t e1 = a.n_counts, e2 = e1 + a.n_acc;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < e2; i += (size_t)gridDim.x * 256) {
    if (i < e1) a.counts[i] = 0u;
    else a.acc[i - e1] = 0ull;
  }
}

// grid (ceil(K / 256), n)
__global__ __launch_bounds__(256) void k_gr_hyp(GrArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (i >= a.K) return;
  const int32_t* raw = a.raw + (size_t)k * a.H * a.W;
  const uint32_t Ns = (uint32_t)a.roi.Ws * (uint32_t)a.roi.Hs;
  int64_t u[3], v[3], r[3];
  bool alive = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t pos = gr_mix(a.seed, 3u * (uint32_t)i + j) % Ns;
    const int sj = (int)(pos % (uint32_t)a.roi.Ws), si = (int)(pos / (uint32_t)a.roi.Ws);
    const int uu = (a.roi.j0 + sj) * a.step, vv = (a.roi.i0 + si) * a.step;
    const int32_t rr = raw[(size_t)vv * a.W + uu];
    alive = alive && gr_usable(rr);
    u[j] = uu, v[j] = vv, r[j] = rr;
  }
  GrHyp hy{0, 0, 0, 0, 0};
  if (alive) {
    const int64_t du1 = u[1] - u[0], dv1 = v[1] - v[0], dr1 = r[1] - r[0], du2 = u[2] - u[0], dv2 = v[2] - v[0], dr2 = r[2] - r[0];
    int64_t A = dv1 * dr2 - dr1 * dv2, B = dr1 * du2 - du1 * dr2, C = du1 * dv2 - dv1 * du2;
    if (C < 0) A = -A, B = -B, C = -C;
    const int64_t D = A * u[0] + B * v[0] + C * r[0];
    alive = C >= a.min_area && C > 0;
    if (alive) {
      const int64_t na = -A * 65536, nb = -B * 65536;
      alive = a.gate[0] * C <= na && na <= a.gate[1] * C && a.gate[2] * C <= nb && nb <= a.gate[3] * C;
      const __int128 nc = (__int128)(D - A * a.roi.u0 - B * a.roi.v0) * 65536;      // 70 bits
      alive = alive && (__int128)a.gate[4] * C <= nc && nc <= (__int128)a.gate[5] * C;
    }
    if (alive) hy = GrHyp{A, B, D, (int32_t)C, 0};
  }
  a.hyp[(size_t)k * a.K + i] = hy;
}

// grid (tiles across * tiles down, n): a tile is a.rows sample rows x 256 sample columns
__global__ __launch_bounds__(256) void k_gr_score(GrArgs a) {
  __shared__ int32_t tile[kGrRows][256];
  __shared__ uint32_t red[4];
  const int k = blockIdx.y, tid = threadIdx.x;
  const int tiles_x = (a.roi.Ws + 255) / 256;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int32_t* raw = a.raw + (size_t)k * a.H * a.W;
  const int col = tx * 256 + tid;
  uint32_t usable = 0;
#pragma unroll
  for (int e = 0; e < kGrRows; ++e) {
    if (e >= a.rows) break;
    const int row = ty * a.rows + e;
    int32_t r = 0;
    if (col < a.roi.Ws && row < a.roi.Hs) r = raw[(size_t)((a.roi.i0 + row) * a.step) * a.W + (size_t)(a.roi.j0 + col) * a.step];
    if (!gr_usable(r)) r = 0;
    usable += r != 0;
    tile[e][tid] = r;
  }
  const uint32_t total = pc_block_sum(usable, red);      // its barriers also publish the tile
  if (tid == 0 && total) atomicAdd(a.acc + (size_t)k * a.acc_words, (unsigned long long)total);
  const int cols = min(256, a.roi.Ws - tx * 256), rows = min(a.rows, a.roi.Hs - ty * a.rows);
  const int Kp = a.K <= 64 ? 64 : (a.K <= 128 ? 128 : 256), parts = 256 / Kp;      // a wave is inside one part
  const int part = tid / Kp, slot = tid - part * Kp;
  const int64_t u_first = (int64_t)(a.roi.j0 + tx * 256) * a.step;
  for (int hb = 0; hb < a.K; hb += 256) {
    const int hi = hb + slot;
    if (hi >= a.K) continue;
    const GrHyp hy = a.hyp[(size_t)k * a.K + hi];
    if (!hy.C) continue;
    // |err| <= tolC as one unsigned compare: 0 <= err + tolC <= 2 tolC (tolC <= 2^51 and |err| < 2^54: nothing wraps)
    const int64_t tolC = a.tol * hy.C, stepA = hy.A * a.step;
    const uint64_t band = 2 * (uint64_t)tolC;
    uint32_t cnt = 0;
    for (int e = part; e < rows; e += parts) {
      const int64_t v = (int64_t)(a.roi.i0 + ty * a.rows + e) * a.step;
      int64_t base = hy.A * u_first + hy.B * v - hy.D + tolC;
      for (int c = 0; c < cols; ++c) {
        const int32_t r = tile[e][c];
        const uint64_t shifted = (uint64_t)(base + (int64_t)hy.C * (int64_t)r);
        cnt += (r != 0) & (shifted <= band);
        base += stepA;
      }
    }
    if (cnt) atomicAdd(a.counts + (size_t)k * a.K + hi, cnt);
  }
}

// grid (n): the winner of map blockIdx.x
__global__ __launch_bounds__(256) void k_gr_select(GrArgs a) {
  __shared__ uint32_t s_cnt[256], s_alive[256];
  __shared__ int s_idx[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  uint32_t best = 0, alive = 0;
  int idx = -1;
  for (int i = tid; i < a.K; i += 256) {
    if (!a.hyp[(size_t)k * a.K + i].C) continue;
    const uint32_t c = a.counts[(size_t)k * a.K + i];
    ++alive;
    if (idx < 0 || c > best) best = c, idx = i;      // a lane's indices rise
  }
  s_cnt[tid] = best, s_idx[tid] = idx, s_alive[tid] = alive;
  __syncthreads();
  if (tid) return;
  for (int t = 1; t < 256; ++t) {
    alive += s_alive[t];
    if (s_idx[t] >= 0 && (idx < 0 || s_cnt[t] > best || (s_cnt[t] == best && s_idx[t] < idx))) best = s_cnt[t], idx = s_idx[t];
  }
  GrState st{{0, 0, 0}, 0, 0, -1, alive};
  if (idx >= 0) {
#pragma clang fp contract(off)
    const GrHyp hy = a.hyp[(size_t)k * a.K + idx];
    const double C = (double)hy.C;
    const int64_t num = hy.D - hy.A * a.roi.u0 - hy.B * a.roi.v0;      // |num| < 2^53: exact in double
    // inside the gate, so inside the limits
    const bool ok = gr_q16((double)(-hy.A) / C, kGrSlopeLim + 1, &st.q[0]) && gr_q16((double)(-hy.B) / C, kGrSlopeLim + 1, &st.q[1]) &&
                    gr_q16((double)num / C, kGrOffsetLim + 1, &st.q[2]);
    st.has = ok, st.winner = idx;
  }
  a.state[k] = st;
}

__device__ __forceinline__ unsigned long long gr_block_sum64(unsigned long long v, unsigned long long* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// grid (tiles, n), tiles of kGrRows sample rows x 256 columns whatever k_gr_score's are (every workgroup sends nine atomics to the
// same nine words of its map, so fewer and larger tiles are the cheaper ones here); round t adds to acc[1 + 9 t ..]
__global__ __launch_bounds__(256) void k_gr_moments(GrArgs a, int round) {
  __shared__ unsigned long long red[4];
  const int k = blockIdx.y, tid = threadIdx.x;
  const GrState st = a.state[k];
  if (!st.has) return;      // the whole workgroup
  const int tiles_x = (a.roi.Ws + 255) / 256;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int32_t* raw = a.raw + (size_t)k * a.H * a.W;
  const int col = tx * 256 + tid;
  const int64_t tol16 = a.tol * 65536;
  int64_t s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (col < a.roi.Ws) {
    const int u = (a.roi.j0 + col) * a.step;
    const int64_t du = u - a.roi.u0;
    for (int e = 0; e < kGrRows; ++e) {
      const int row = ty * kGrRows + e;
      if (row >= a.roi.Hs) break;
      const int v = (a.roi.i0 + row) * a.step;
      const int32_t r32 = raw[(size_t)v * a.W + u];
      if (!gr_usable(r32)) continue;
      const int64_t dv = v - a.roi.v0, r = r32;
      const int64_t err = r * 65536 - (st.q[0] * du + st.q[1] * dv + st.q[2]);
      if (gr_abs(err) > tol16) continue;
      s[0] += 1, s[1] += du, s[2] += dv, s[3] += r, s[4] += du * du, s[5] += du * dv, s[6] += dv * dv, s[7] += du * r, s[8] += dv * r;
    }
  }
  unsigned long long* acc = a.acc + (size_t)k * a.acc_words + 1 + 9 * round;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const unsigned long long total = gr_block_sum64((unsigned long long)s[q], red);      // two's complement: the sum wraps back
    if (tid == 0 && total) atomicAdd(acc + q, total);
  }
}

// grid (ceil(n / 64)): a lane per map, round t's moments -> the next plane
__global__ __launch_bounds__(64) void k_gr_solve(GrArgs a, int round) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= a.n) return;
  GrState st = a.state[k];
  if (!st.has || st.stop) return;
  const unsigned long long* acc = a.acc + (size_t)k * a.acc_words + 1 + 9 * round;
  const int64_t N = (int64_t)acc[0];
  bool ok = N >= 3;
  int64_t q[3] = {0, 0, 0};
  if (ok) {
    const double n = (double)N, Su = (double)(int64_t)acc[1], Sv = (double)(int64_t)acc[2], Sr = (double)(int64_t)acc[3];
    const double Suu = (double)(int64_t)acc[4], Suv = (double)(int64_t)acc[5], Svv = (double)(int64_t)acc[6];
    const double Sur = (double)(int64_t)acc[7], Svr = (double)(int64_t)acc[8];
    const double mu = Su / n, mv = Sv / n, mr = Sr / n;
    const double suu = Suu - Su * mu, suv = Suv - Su * mv, svv = Svv - Sv * mv, sur = Sur - Su * mr, svr = Svr - Sv * mr;
    const double det = suu * svv - suv * suv;
    ok = det > 0.0;
    if (ok) {
      const double pa = (sur * svv - svr * suv) / det, pb = (svr * suu - sur * suv) / det;
      const double pc = (mr - pa * mu) - pb * mv;
      ok = gr_q16(pa, kGrSlopeLim, &q[0]) && gr_q16(pb, kGrSlopeLim, &q[1]) && gr_q16(pc, kGrOffsetLim, &q[2]);
    }
  }
  if (ok) st.q[0] = q[0], st.q[1] = q[1], st.q[2] = q[2];
  else st.stop = 1;
  a.state[k] = st;
}

// grid (ceil(n / 64)): a lane per map
__global__ __launch_bounds__(64) void k_gr_finish(GrArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= a.n) return;
  const GrState st = a.state[k];
  const unsigned long long* acc = a.acc + (size_t)k * a.acc_words;
  const uint32_t inliers = st.has ? (uint32_t)acc[1 + 9 * a.refits] : 0u;
  uint32_t flags = st.stop ? SN_GROUND_SINGULAR : 0u;
  if (!st.has) flags |= SN_GROUND_NO_HYPOTHESIS;
  else if (inliers < (uint32_t)a.min_inliers) flags |= SN_GROUND_FEW_INLIERS;
  float plane[4] = {-a.m[8], -a.m[9], -a.m[10], a.m[11]}, mount[12];
  for (int e = 0; e < 12; ++e) mount[e] = a.m[e];
  if (st.has && !(flags & SN_GROUND_FEW_INLIERS)) {
    bool in = a.gate[0] <= st.q[0] && st.q[0] <= a.gate[1] && a.gate[2] <= st.q[1] && st.q[1] <= a.gate[3] && a.gate[4] <= st.q[2] &&
              st.q[2] <= a.gate[5];
    const double pa = (double)st.q[0] / 65536.0, pb = (double)st.q[1] / 65536.0, pc = (double)st.q[2] / 65536.0;
    const double fx = (double)a.fx, fy = (double)a.fy;
    const double cp = (pc + pa * ((double)a.cx - (double)a.roi.u0)) + pb * ((double)a.cy - (double)a.roi.v0);
    const double w0 = pa, w1 = (pb * fy) / fx, w2 = cp / fx;
    const double len = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    in = in && len > 0.0 && len < INFINITY;
    double hgt = 0.0, z[3] = {0, 0, 0}, x[3] = {0, 0, 0};
    if (in) {
      hgt = ((double)a.baseline_mm / 1000.0) / ((double)a.S * len);
      z[0] = -(w0 / len), z[1] = -(w1 / len), z[2] = -(w2 / len);
      const double p0 = (double)a.m[0], p1 = (double)a.m[1], p2 = (double)a.m[2];
      const double d = (p0 * z[0] + p1 * z[1]) + p2 * z[2];
      x[0] = p0 - d * z[0], x[1] = p1 - d * z[1], x[2] = p2 - d * z[2];
      const double xl = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
      in = xl >= 1e-3;
      if (in) x[0] = x[0] / xl, x[1] = x[1] / xl, x[2] = x[2] / xl;
    }
    if (in) {
      const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
      for (int e = 0; e < 3; ++e) {
        plane[e] = (float)-z[e];
        mount[e] = (float)x[e], mount[4 + e] = (float)y[e], mount[8 + e] = (float)z[e];
      }
      plane[3] = (float)hgt, mount[11] = (float)hgt;
      flags |= SN_GROUND_FOUND;
    } else {
      flags |= SN_GROUND_GATED;
    }
  }
  sn_ground g;
  g.flags = flags, g.usable = (uint32_t)acc[0], g.inliers = inliers, g.winner = st.winner, g.survivors = st.survivors, g.reserved = 0;
  for (int e = 0; e < 3; ++e) g.plane_q16[e] = st.q[e];
  for (int e = 0; e < 4; ++e) g.plane_cam[e] = plane[e];
  for (int e = 0; e < 12; ++e) g.base_from_cam[e] = mount[e];
  a.out[k] = g;
}

__device__ __forceinline__ uint32_t gr_label(int32_t r32, int64_t pred, int64_t tol16, bool plane) {
  if (!gr_usable(r32)) return SN_GROUND_LABEL_NONE;
  if (!plane) return SN_GROUND_LABEL_NO_PLANE;
  const int64_t err = (int64_t)r32 * 65536 - pred;
  return gr_abs(err) <= tol16 ? SN_GROUND_LABEL_GROUND : (err > 0 ? SN_GROUND_LABEL_ABOVE : SN_GROUND_LABEL_BELOW);
}

// grid (workgroups per map, n).  VEC: the map is 16-byte aligned, the labels 4-byte, H * W a multiple of 4: a lane takes four
// consecutive pixels (which may cross a row's end)
template <bool VEC>
__global__ __launch_bounds__(256) void k_gr_labels(GrArgs a) {
  const int k = blockIdx.y;
  const sn_ground* g = a.out + k;
  const bool plane = (g->flags & SN_GROUND_FOUND) != 0;
  const int64_t qa = g->plane_q16[0], qb = g->plane_q16[1], qc = g->plane_q16[2], tol16 = a.tol * 65536;
  const size_t HW = (size_t)a.H * a.W;
  const int32_t* raw = a.raw + (size_t)k * HW;
  uint8_t* lab = a.labels + (size_t)k * HW;
  if (VEC) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < HW / 4; q += (size_t)gridDim.x * 256) {
      const int4 r4 = *reinterpret_cast<const int4*>(raw + 4 * q);
      const int32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
      int v = (int)(4 * q / a.W), u = (int)(4 * q - (size_t)v * a.W);
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t pred = qa * (u - a.roi.u0) + qb * (v - a.roi.v0) + qc;
        word |= gr_label(r[e], pred, tol16, plane) << (8 * e);
        if (++u == a.W) u = 0, ++v;
      }
      *reinterpret_cast<uint32_t*>(lab + 4 * q) = word;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
      const int v = (int)(i / a.W), u = (int)(i - (size_t)v * a.W);
      const int64_t pred = qa * (u - a.roi.u0) + qb * (v - a.roi.v0) + qc;
      lab[i] = (uint8_t)gr_label(raw[i], pred, tol16, plane);
    }
  }
}

}  // namespace sn
