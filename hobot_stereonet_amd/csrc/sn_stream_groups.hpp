// sn_stream_groups.hpp — what the stages with per-stream state (temporal filter, costmap, elevation map) share on the host: the
// group lists that travel in the kernel arguments, how a slice of a push is sorted into them, what a stream keeps once the
// slice is enqueued, and the pose rule of the two rolling maps.  Plain C++: no HIP header and no handle, so that a host
// compiler can build it alone (csrc/compat/test/stream_groups_check.cpp runs it under the sanitizers).
#pragma once
#include <cmath>
#include <stdint.h>

namespace sn {

constexpr int kSlice = 64;      // maps per launch: the per-stream frame lists (and a torus's poses) travel in the kernel arguments

// The maps of a slice sorted by stream: group g owns map[first[g] .. first[g + 1]), in time order, and updates one state.
struct StreamGroups {
  int first[kSlice + 1];
  int stream[kSlice];      // per group: which state it updates
  int fresh[kSlice];       // per group: no frame since create / reset, so the kernel reads no state
  int map[kSlice];         // map indices of the slice, grouped by stream, each group in the order of k
};

// What a torus adds per group: the origin of the stream's previous frame (unless fresh)
struct TorusPrev {
  int pox[kSlice], poy[kSlice];
};

// Groups maps k0 .. k0 + m of a push (m <= kSlice) by stream, in order of first appearance, each in the order of k; stream_of ==
// nullptr: all on stream 0.  Returns the number of groups; last[g] is group g's last map of the slice.
inline int group_slice(StreamGroups& a, int* last, const int* stream_of, int k0, int m, const uint8_t* fresh) {
  int groups = 0, filled = 0;
  for (int k = 0; k < m; ++k) {
    const int id = stream_of ? stream_of[k0 + k] : 0;
    bool known = false;
    for (int g = 0; g < groups && !known; ++g) known = a.stream[g] == id;
    if (!known) a.stream[groups++] = id;
  }
  for (int g = 0; g < groups; ++g) {
    const int id = a.stream[g];
    a.first[g] = filled;
    a.fresh[g] = fresh[id];
    for (int k = 0; k < m; ++k)
      if ((stream_of ? stream_of[k0 + k] : 0) == id) a.map[filled++] = k, last[g] = k;
  }
  a.first[groups] = filled;
  return groups;
}

// ... and, for a torus, each group's previous origin
inline int group_slice(StreamGroups& a, TorusPrev& t, int* last, const int* stream_of, int k0, int m, const uint8_t* fresh,
                       const int* ox, const int* oy) {
  const int groups = group_slice(a, last, stream_of, k0, m, fresh);
  for (int g = 0; g < groups; ++g) t.pox[g] = ox[a.stream[g]], t.poy[g] = oy[a.stream[g]];
  return groups;
}

// The slice is enqueued: the state now holds these frames
inline void commit_slice(const StreamGroups& a, int groups, uint8_t* fresh) {
  for (int g = 0; g < groups; ++g) fresh[a.stream[g]] = 0;
}

// ... and a torus stream keeps the origin of its last frame; q: per map of the slice tx, ty, cq, sq, ox, oy
inline void commit_slice(const StreamGroups& a, int groups, const int* last, const int (*q)[6], uint8_t* fresh, int* ox, int* oy) {
  commit_slice(a, groups, fresh);
  for (int g = 0; g < groups; ++g) ox[a.stream[g]] = q[last[g]][4], oy[a.stream[g]] = q[last[g]][5];
}

// The contract's q of one pose (x, y, yaw) for a window of mw x mh cells of 256 subs, k256 subs a metre; false where
// sn_costmap_pose_q and sn_elevation_pose_q refuse it: a field that is not finite, or |x * k256| or |y * k256| above 2^30
inline bool torus_pose_q(double k256, int mw, int mh, const double* pose, int32_t* q) {
  const double x = pose[0], y = pose[1], yaw = pose[2], lim = 1073741824.0;
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(yaw)) return false;
  const double fx = x * k256, fy = y * k256;
  if (!(std::fabs(fx) <= lim) || !(std::fabs(fy) <= lim)) return false;
  const long long tx = std::llrint(fx), ty = std::llrint(fy);
  q[0] = (int32_t)tx, q[1] = (int32_t)ty;
  q[2] = (int32_t)std::llrint(std::cos(yaw) * lim), q[3] = (int32_t)std::llrint(std::sin(yaw) * lim);
  q[4] = (int32_t)((tx >> 8) - mw / 2), q[5] = (int32_t)((ty >> 8) - mh / 2);
  return true;
}

}  // namespace sn
