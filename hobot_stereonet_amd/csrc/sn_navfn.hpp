// sn_navfn.hpp — the navigation function and the path to a goal over inflated cost grids (sn_navfn; the contract is in
// include/stereonet_hip.h, the numpy twin is hobot_stereonet_amd/navfn.py).  Everything is integer, and the field is the unique
// fixed point of min-plus relaxation, so the schedule below may be as loose as it likes: whatever converges gives the same words.
//
// A tiled, asynchronous Bellman-Ford.  The launch boundary is the only grid-wide synchronisation: no workgroup waits for
// another, no barrier spans workgroups, nothing is persistent (DESIGN §5t has the argument for the round bound).
//
//   k_nav_init    grid (cells / 256, maps).  P = 0xFFFFFFFF everywhere but 0 at a passable goal, whose tile and the eight around
//                 it are marked active for round 0; counts the blocked cells and sets SN_NAV_GOAL_BLOCKED.
//   k_nav_relax   grid (tiles of a map, maps), 1024 threads: a workgroup owns one 32 x 32 tile of one map, a thread one cell.
//                 A workgroup whose tile is not marked for this round leaves after one load.  Otherwise it reads its tile of P
//                 and of the weights with a one-cell halo into LDS (34 x 34 words: a row of 32 consecutive words per half wave,
//                 no bank conflict) and relaxes in LDS, the halo held fixed, until a sweep changes no cell (__syncthreads_or; at
//                 most kNavMaxSweeps sweeps, see there).  A cell that ended lower than it was loaded is stored: the interior of
//                 a tile has exactly one writer, so P needs no atomics.  For every side or corner on which a border cell ended
//                 lower, that neighbouring tile is marked for the NEXT round.  Marks are double-buffered by the round's parity
//                 and the reader of a round clears its own.
//                 A tile may read a neighbour's border while the neighbour stores it in the same launch.  It sees the old or the
//                 new aligned 32-bit word; both are costs of real routes, so both are valid upper bounds, and because the writer
//                 marks the reader for the next round the new word is not lost.
//                 Values only ever fall, and every stored word is the cost of a route without a repeated cell (a candidate
//                 through a cell's own older value exceeds its current one and is refused), which bounds it as the header says.
//   k_nav_stats   grid (cells / 256, maps): the cells with a finite P, and SN_NAV_UNCONVERGED from the marks left for the round
//                 that was not run.
//   k_nav_path    grid (maps), one wave: lanes 0..7 evaluate the eight neighbours of the current cell, the minimum of a packed
//                 (value << 3 | order) key picks the move.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stereonet_hip.h"

namespace sn {

constexpr int kNavTW = SN_NAV_TILE_W, kNavTH = SN_NAV_TILE_H;
constexpr int kNavLW = kNavTW + 2, kNavLH = kNavTH + 2;      // the tile with its halo
constexpr int kNavThreads = kNavTW * kNavTH;
static_assert(kNavThreads == 1024 && kNavTW == 32, "k_nav_relax maps a thread to a cell by shifts of 5");
// Sweeps of one visit to a tile.  With the halo fixed, sweep s settles every cell whose cheapest way to the halo (or the goal)
// has at most s moves inside the tile; such a way repeats no cell, so it has at most kNavTW * kNavTH moves, and one more sweep
// sees no change.  The bound is the cells of the tile plus its halo; a visit that ever reached it would mark its own tile again.
constexpr int kNavMaxSweeps = kNavLW * kNavLH;
constexpr int kNavMaxSide = 4096;        // gw, gh (their product: SN_NAV_MAX_CELLS)
constexpr int kNavChunk = 8;             // max_rounds == 0: rounds enqueued between two reads of the work word

// nullptr, or why sn_navfn refuses the parameters
inline const char* nav_params_check(const sn_nav_params* p) {
  if (!p) return "a NULL pointer";
  if (p->neutral < 1 || p->neutral > 255) return "neutral must be 1..255";
  if (p->lethal_cost < 1 || p->lethal_cost > 255) return "lethal_cost must be 1..255";
  if (p->unknown_cost < 0 || p->unknown_cost > 252) return "unknown_cost must be 0..252";
  if (p->flags & ~SN_NAV_UNKNOWN_OK) return "flags has bits other than SN_NAV_UNKNOWN_OK";
  if (p->max_rounds < 0) return "max_rounds must not be negative";
  if (p->max_path < 0) return "max_path must not be negative";
  return nullptr;
}

struct NavArgs {
  const uint8_t* cost;      // [maps][gh][gw]
  const int32_t* goals;     // [maps][2]
  const int32_t* starts;    // nullable
  uint32_t* pot;            // [maps][gh][gw]
  int32_t* path;            // nullable: [maps][max_path][2]
  uint32_t* stats;          // nullable: [maps][5], zeroed before k_nav_init
  uint32_t* marks;          // [2][maps][tiles], zeroed before k_nav_init
  uint32_t* work;           // one word, zeroed before k_nav_init: 1 + the last round in which a tile was active
  int gw, gh, tiles_x, tiles_y, maps;
  int neutral, lethal, unknown_cost, flags, max_path;
};

// the eight neighbours in the order of the contract: E, NE, N, NW, W, SW, S, SE (north is y - 1); odd = diagonal
__host__ __device__ __forceinline__ int nav_dx(int d) { return (d == 0 || d == 1 || d == 7) - (d >= 3 && d <= 5); }
__host__ __device__ __forceinline__ int nav_dy(int d) { return (d >= 5 && d <= 7) - (d >= 1 && d <= 3); }

// w of a cell, 0 where it is blocked
__device__ __forceinline__ uint32_t nav_weight(const NavArgs& a, int c) {
  if (c == 255) return (a.flags & SN_NAV_UNKNOWN_OK) ? (uint32_t)(a.neutral + a.unknown_cost) : 0u;
  return c >= a.lethal ? 0u : (uint32_t)(a.neutral + c);
}

__global__ __launch_bounds__(256) void k_nav_init(NavArgs a) {
  const int cells = a.gw * a.gh, map = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < cells;
  const uint8_t* cost = a.cost + (size_t)map * cells;
  const int gx = a.goals[2 * map], gy = a.goals[2 * map + 1];
  const bool goal_in = gx >= 0 && gx < a.gw && gy >= 0 && gy < a.gh;
  const int gi = goal_in ? gy * a.gw + gx : -1;
  const uint32_t w = live ? nav_weight(a, cost[i]) : 0u;
  if (live) {
    const bool goal = i == gi && w;
    a.pot[(size_t)map * cells + i] = goal ? 0u : SN_NAV_INF;
    if (goal) {
      // parity 0.  The goal's word is already final, so its tile's visit never sees it fall and would not mark the tiles that
      // hold the goal in their halo: they are marked here, the tile and the eight around it.
      uint32_t* marks = a.marks + (size_t)map * a.tiles_x * a.tiles_y;
      const int tx = gx / kNavTW, ty = gy / kNavTH;
      for (int ny = max(ty - 1, 0); ny <= min(ty + 1, a.tiles_y - 1); ++ny)
        for (int nx = max(tx - 1, 0); nx <= min(tx + 1, a.tiles_x - 1); ++nx) marks[ny * a.tiles_x + nx] = 1u;
    }
  }
  if (a.stats) {
    const uint32_t blocked = __popcll(__ballot(live && !w));
    if ((threadIdx.x & 63) == 0 && blocked) atomicAdd(a.stats + (size_t)map * 5 + 4, blocked);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !(goal_in && nav_weight(a, cost[gi])))
      atomicOr(a.stats + (size_t)map * 5, (uint32_t)SN_NAV_GOAL_BLOCKED);
  }
}

__global__ __launch_bounds__(kNavThreads) void k_nav_relax(NavArgs a, int round) {
  __shared__ uint32_t P[kNavLH][kNavLW];
  __shared__ uint16_t Wt[kNavLH][kNavLW];
  __shared__ uint32_t s_active, s_touch;
  const int tiles = a.tiles_x * a.tiles_y, tile = blockIdx.x, map = blockIdx.y, tid = threadIdx.x;
  uint32_t* cur = a.marks + ((size_t)(round & 1) * a.maps + map) * tiles;
  uint32_t* nxt = a.marks + ((size_t)((round + 1) & 1) * a.maps + map) * tiles;
  if (tid == 0) {
    s_active = cur[tile];
    if (s_active) cur[tile] = 0u;      // nobody else touches this round's marks: the writers of this launch write the other parity
    s_touch = 0u;
  }
  __syncthreads();
  if (!s_active) return;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int x0 = tx * kNavTW, y0 = ty * kNavTH, cells = a.gw * a.gh;
  const uint8_t* cost = a.cost + (size_t)map * cells;
  uint32_t* pot = a.pot + (size_t)map * cells;
  for (int i = tid; i < kNavLW * kNavLH; i += kNavThreads) {
    const int ly = i / kNavLW, lx = i - ly * kNavLW, x = x0 - 1 + lx, y = y0 - 1 + ly;
    const bool in = x >= 0 && x < a.gw && y >= 0 && y < a.gh;
    const int at = in ? y * a.gw + x : 0;
    const uint32_t w = nav_weight(a, cost[at]);
    const uint32_t p = pot[at];      // of a neighbour's border: the old or the new word, see above
    P[ly][lx] = in ? p : SN_NAV_INF;
    Wt[ly][lx] = (uint16_t)(in ? w : 0u);
  }
  __syncthreads();
  const int lx = tid & 31, ly = tid >> 5, cx = lx + 1, cy = ly + 1;
  const uint32_t wme = Wt[cy][cx];
  unsigned allowed = 0;      // the moves out of this cell, by order index
  if (wme) {
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int ax = cx + nav_dx(d), ay = cy + nav_dy(d);
      bool ok = Wt[ay][ax] != 0;
      if (d & 1) ok = ok && Wt[cy][ax] != 0 && Wt[ay][cx] != 0;
      allowed |= (unsigned)ok << d;
    }
  }
  const uint32_t loaded = P[cy][cx], k5 = 5u * wme, k7 = 7u * wme;
  uint32_t mine = loaded;
  bool more = true;
  for (int sweep = 0; sweep < kNavMaxSweeps; ++sweep) {
    // all eight reads first (the halo makes every one of them a cell of the LDS tile), then the arithmetic: one LDS latency a
    // sweep and no branch
    uint32_t pa[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) pa[d] = P[cy + nav_dy(d)][cx + nav_dx(d)];      // may be rewritten during this sweep: either word will do
    uint32_t best = mine;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const uint32_t cand = pa[d] + ((d & 1) ? k7 : k5);      // no overflow where pa is finite: the header's bound
      best = min(best, (pa[d] != SN_NAV_INF && (allowed >> d & 1)) ? cand : SN_NAV_INF);
    }
    const bool fell = best < mine;
    if (fell) {
      mine = best;
      P[cy][cx] = mine;
    }
    if (!__syncthreads_or(fell)) {
      more = false;
      break;
    }
  }
  if (mine != loaded) {      // a passable cell inside the grid
    pot[(y0 + ly) * a.gw + x0 + lx] = mine;
    const bool e = lx == kNavTW - 1, w = lx == 0, n = ly == 0, s = ly == kNavTH - 1;
    const unsigned touch = (unsigned)e | (unsigned)(e && n) << 1 | (unsigned)n << 2 | (unsigned)(n && w) << 3 | (unsigned)w << 4 |
                           (unsigned)(w && s) << 5 | (unsigned)s << 6 | (unsigned)(s && e) << 7;
    if (touch) atomicOr(&s_touch, touch);
  }
  __syncthreads();
  if (tid < 8 && (s_touch >> tid & 1)) {
    const int ntx = tx + nav_dx(tid), nty = ty + nav_dy(tid);
    if (ntx >= 0 && ntx < a.tiles_x && nty >= 0 && nty < a.tiles_y) nxt[nty * a.tiles_x + ntx] = 1u;
  }
  if (tid == 0) {
    if (more) nxt[tile] = 1u;
    atomicMax(a.work, (uint32_t)round + 1u);
  }
}

// rounds: how many relaxation launches ran; their successor's marks are what is left
__global__ __launch_bounds__(256) void k_nav_stats(NavArgs a, int rounds, int fixed_rounds) {
  const int cells = a.gw * a.gh, map = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t finite = __popcll(__ballot(i < cells && a.pot[(size_t)map * cells + (i < cells ? i : 0)] != SN_NAV_INF));
  uint32_t* stats = a.stats + (size_t)map * 5;
  if ((threadIdx.x & 63) == 0 && finite) atomicAdd(stats + 1, finite);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0 && !a.starts) stats[3] = SN_NAV_INF;
    if (fixed_rounds) {
      const int tiles = a.tiles_x * a.tiles_y;
      const uint32_t* left = a.marks + ((size_t)(rounds & 1) * a.maps + map) * tiles;
      bool any = false;
      for (int t = threadIdx.x; t < tiles; t += 256) any = any || left[t] != 0u;
      if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(stats, (uint32_t)SN_NAV_UNCONVERGED);
    }
  }
}

// grid (maps), 64 threads
__global__ __launch_bounds__(64) void k_nav_path(NavArgs a) {
  const int cells = a.gw * a.gh, map = blockIdx.x, lane = threadIdx.x;
  const uint8_t* cost = a.cost + (size_t)map * cells;
  const uint32_t* pot = a.pot + (size_t)map * cells;
  int32_t* path = a.path ? a.path + (size_t)map * a.max_path * 2 : nullptr;
  int cx = a.starts[2 * map], cy = a.starts[2 * map + 1];
  uint32_t flags = 0, len = 0, pstart = SN_NAV_INF;
  if (cx >= 0 && cx < a.gw && cy >= 0 && cy < a.gh) pstart = pot[cy * a.gw + cx];
  if (pstart == SN_NAV_INF) {
    flags |= SN_NAV_START_UNREACHABLE;
  } else {
    // P strictly decreases along the path, so it has at most `cells` cells; only the first max_path of them are written, but all
    // are counted (the contract reports the full length), so the loop's bound is the grid, not max_path: one wave, a round of
    // dependent loads a step, about a microsecond each, so the longest route of a 2^20-cell maze keeps it busy for half a second
    // P and w of the current cell travel with the walk (a lane has loaded both for the neighbour that is taken), so a step
    // waits for one round of loads, the neighbours'
    uint32_t pc = pstart, wc = nav_weight(a, cost[cy * a.gw + cx]);
    for (int step = 0; step < cells; ++step) {
      if (path && len < (uint32_t)a.max_path && lane == 0) path[2 * len] = cx, path[2 * len + 1] = cy;
      ++len;
      if (pc == 0u) break;      // w >= 1: the goal alone holds 0
      unsigned long long key = ~0ull;
      uint32_t pa = SN_NAV_INF, wa = 0u;
      if (lane < 8) {
        const int ax = cx + nav_dx(lane), ay = cy + nav_dy(lane);
        if (ax >= 0 && ax < a.gw && ay >= 0 && ay < a.gh) {
          pa = pot[ay * a.gw + ax];
          wa = nav_weight(a, cost[ay * a.gw + ax]);
          bool ok = wa != 0u;
          if (lane & 1) ok = ok && nav_weight(a, cost[cy * a.gw + ax]) != 0u && nav_weight(a, cost[ay * a.gw + cx]) != 0u;
          if (ok && pa != SN_NAV_INF) key = (unsigned long long)(pa + ((lane & 1) ? 7u : 5u) * wc) << 3 | (unsigned)lane;
        }
      }
#pragma unroll
      for (int off = 4; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other < key ? other : key;
      }
      key = __shfl(key, 0);
      if (key == ~0ull) break;      // a finite cell other than the goal always has a finite neighbour
      const int d = (int)(key & 7);
      pc = __shfl(pa, d), wc = __shfl(wa, d);
      cx += nav_dx(d), cy += nav_dy(d);
    }
    if (path && len > (uint32_t)a.max_path) flags |= SN_NAV_PATH_TRUNCATED;
  }
  if (lane == 0 && a.stats) {
    uint32_t* stats = a.stats + (size_t)map * 5;
    if (flags) atomicOr(stats, flags);
    stats[2] = len;
    stats[3] = pstart;
  }
}

}  // namespace sn
