// stream_groups_check — the pure-host pieces of the stream and torus layer (csrc/sn_stream_groups.hpp: the grouping of a slice,
// its commit, the pose rule) against a restatement written here, under AddressSanitizer and UndefinedBehaviorSanitizer
// (make stream_groups_check).  No GPU, no library: exit status 0 means every case agreed and the sanitizers saw nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../../sn_stream_groups.hpp"

namespace {

int failures = 0;

#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);              \
      std::fprintf(stderr, "\n");                     \
    }                                                 \
  } while (0)

// The host's state of a torus object, and the restatement's copy of it
struct State {
  std::vector<uint8_t> fresh;
  std::vector<int> ox, oy;
  explicit State(int streams) : fresh(streams, 1), ox(streams, 0), oy(streams, 0) {}
};

int id_of(const int* stream_of, int k) { return stream_of ? stream_of[k] : 0; }

// One slice through group_slice and commit_slice, held to buckets filled in one pass over k.  The arguments live on the heap
// at their exact size, so an index past either end is the sanitizer's.
void run_slice(const char* what, const int* stream_of, int k0, int m, const std::vector<int>& q_all, State& got, State& want, bool torus) {
  std::unique_ptr<sn::StreamGroups> g(new sn::StreamGroups);
  std::unique_ptr<sn::TorusPrev> t(new sn::TorusPrev);
  std::vector<int> last(m, -1);
  const int groups = torus ? sn::group_slice(*g, *t, last.data(), stream_of, k0, m, got.fresh.data(), got.ox.data(), got.oy.data())
                           : sn::group_slice(*g, last.data(), stream_of, k0, m, got.fresh.data());
  std::vector<int> order;                    // streams in order of first appearance
  std::vector<std::vector<int>> bucket;      // per stream of `order`: its maps, in the order of k
  for (int k = 0; k < m; ++k) {
    const int id = id_of(stream_of, k0 + k);
    size_t at = 0;
    while (at < order.size() && order[at] != id) ++at;
    if (at == order.size()) order.push_back(id), bucket.emplace_back();
    bucket[at].push_back(k);
  }
  CHECK(groups == (int)order.size(), "%s: %d groups, expected %zu", what, groups, order.size());
  if (groups != (int)order.size()) return;
  int filled = 0;
  for (int gi = 0; gi < groups; ++gi) {
    const int id = order[gi];
    CHECK(g->stream[gi] == id, "%s: group %d is stream %d, expected %d", what, gi, g->stream[gi], id);
    CHECK(g->first[gi] == filled, "%s: first[%d] = %d, expected %d", what, gi, g->first[gi], filled);
    CHECK(g->fresh[gi] == want.fresh[id], "%s: fresh[%d] = %d, expected %d", what, gi, g->fresh[gi], want.fresh[id]);
    if (torus) CHECK(t->pox[gi] == want.ox[id] && t->poy[gi] == want.oy[id], "%s: group %d previous origin (%d, %d), expected (%d, %d)", what, gi, t->pox[gi], t->poy[gi], want.ox[id], want.oy[id]);
    for (int k : bucket[gi]) {
      CHECK(g->map[filled] == k, "%s: map[%d] = %d, expected %d", what, filled, g->map[filled], k);
      ++filled;
    }
    CHECK(last[gi] == bucket[gi].back(), "%s: last[%d] = %d, expected %d", what, gi, last[gi], bucket[gi].back());
  }
  CHECK(g->first[groups] == m && filled == m, "%s: first[groups] = %d, expected %d", what, g->first[groups], m);
  // the commit: every stream of the slice has seen a frame, and a torus keeps the origin of its last map
  const int(*q)[6] = reinterpret_cast<const int(*)[6]>(q_all.data() + (size_t)k0 * 6);
  if (torus) sn::commit_slice(*g, groups, last.data(), q, got.fresh.data(), got.ox.data(), got.oy.data());
  else sn::commit_slice(*g, groups, got.fresh.data());
  for (int k = 0; k < m; ++k) {
    const int id = id_of(stream_of, k0 + k);
    want.fresh[id] = 0;
    if (torus) want.ox[id] = q_all[(size_t)(k0 + k) * 6 + 4], want.oy[id] = q_all[(size_t)(k0 + k) * 6 + 5];
  }
  CHECK(got.fresh == want.fresh, "%s: the fresh flags after the commit differ", what);
  CHECK(got.ox == want.ox && got.oy == want.oy, "%s: the origins after the commit differ", what);
}

void check_grouper() {
  const int sizes[] = {1, 2, 63, 64}, stream_counts[] = {1, 3, 64};
  char what[128];
  for (int torus = 0; torus < 2; ++torus)
    for (int streams : stream_counts)
      for (int m : sizes)
        for (int pattern = 0; pattern < 5; ++pattern) {
          // two slices' worth of maps: the second slice (k0 = 64) sees what the commit of the first left
          const int n = sn::kSlice + m;
          std::vector<int> ids(n), q((size_t)n * 6);
          for (int k = 0; k < n; ++k) {
            switch (pattern) {
              case 0: ids[k] = streams - 1; break;                         // all on one stream
              case 1: ids[k] = k % streams; break;                         // every map on its own stream (streams >= m), else round robin
              case 2: ids[k] = (k * 7 + 3) % streams; break;               // interleaved
              case 3: ids[k] = (streams - 1) - (k / 2) % streams; break;   // pairs, streams in descending order
              default: break;                                              // stream_of == nullptr
            }
            for (int e = 0; e < 6; ++e) q[(size_t)k * 6 + e] = 1000 * k + e - 5000;
          }
          const int* stream_of = pattern == 4 ? nullptr : ids.data();
          State got(streams), want(streams);
          std::snprintf(what, sizeof what, "%s, %d streams, pattern %d, a slice of %d", torus ? "torus" : "plain", streams, pattern, m);
          State got1(streams), want1(streams);
          run_slice(what, stream_of, 0, m, q, got1, want1, torus != 0);      // a first slice of m maps alone
          std::snprintf(what, sizeof what, "%s, %d streams, pattern %d, 64 maps then %d", torus ? "torus" : "plain", streams, pattern, m);
          run_slice(what, stream_of, 0, sn::kSlice, q, got, want, torus != 0);
          run_slice(what, stream_of, sn::kSlice, m, q, got, want, torus != 0);
        }
}

// the rule of include/stereonet_hip.h, restated: floor division written out, the limits as comparisons of the products
bool pose_expected(double k256, int mw, int mh, const double* pose, long long* q) {
  for (int e = 0; e < 3; ++e)
    if (pose[e] != pose[e] || pose[e] == std::numeric_limits<double>::infinity() || pose[e] == -std::numeric_limits<double>::infinity()) return false;
  const double lim = std::ldexp(1.0, 30), fx = pose[0] * k256, fy = pose[1] * k256;
  if (fx > lim || fx < -lim || fy > lim || fy < -lim || fx != fx || fy != fy) return false;
  const long long tx = (long long)std::nearbyint(fx), ty = (long long)std::nearbyint(fy);      // round to nearest, ties to even
  auto floor256 = [](long long v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); };
  q[0] = tx, q[1] = ty;
  q[2] = (long long)std::nearbyint(std::cos(pose[2]) * lim), q[3] = (long long)std::nearbyint(std::sin(pose[2]) * lim);
  q[4] = floor256(tx) - mw / 2, q[5] = floor256(ty) - mh / 2;
  return true;
}

void check_pose(double k256, int mw, int mh, double x, double y, double yaw) {
  const double pose[3] = {x, y, yaw};
  std::unique_ptr<int32_t[]> q(new int32_t[6]);
  for (int e = 0; e < 6; ++e) q[e] = -77;
  long long want[6];
  const bool ok = sn::torus_pose_q(k256, mw, mh, pose, q.get()), ok_want = pose_expected(k256, mw, mh, pose, want);
  CHECK(ok == ok_want, "pose (%a, %a, %a) k256 %a: %s, expected %s", x, y, yaw, k256, ok ? "accepted" : "refused", ok_want ? "accepted" : "refused");
  if (!ok || !ok_want) return;
  for (int e = 0; e < 6; ++e)
    CHECK(q[e] == want[e], "pose (%a, %a, %a) k256 %a window %d x %d: q[%d] = %d, expected %lld", x, y, yaw, k256, mw, mh, e, q[e], want[e]);
}

void check_pose_rule() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int windows[][2] = {{1, 1}, {2, 2}, {7, 4}, {4, 7}, {255, 256}, {4096, 4095}};
  const double k256s[] = {256.0, 256.0 / 0.05, 256.0 / (double)0.1f, 256.0 / 3.0};
  for (const auto& w : windows)
    for (double k256 : k256s) {
      const int mw = w[0], mh = w[1];
      // |x * k256| = 2^30 exactly is accepted, the next double above it is refused; the edge is sought on the product
      double edge = std::ldexp(1.0, 30) / k256;
      while (edge * k256 > std::ldexp(1.0, 30)) edge = std::nextafter(edge, 0.0);
      while (std::nextafter(edge, inf) * k256 <= std::ldexp(1.0, 30)) edge = std::nextafter(edge, inf);
      const double over = std::nextafter(edge, inf);
      for (double s : {1.0, -1.0}) {
        check_pose(k256, mw, mh, s * edge, 0.25, 0.5);
        check_pose(k256, mw, mh, s * over, 0.25, 0.5);
        check_pose(k256, mw, mh, -0.25, s * edge, -2.5);
        check_pose(k256, mw, mh, -0.25, s * over, -2.5);
      }
      if (k256 == 256.0) {      // a cell of one metre: the edge is 2^22 m and the product is exact
        int32_t q[6];
        const double at[3] = {4194304.0, -4194304.0, 0.0}, past[3] = {std::nextafter(4194304.0, inf), 0.0, 0.0};
        CHECK(sn::torus_pose_q(k256, mw, mh, at, q) && q[0] == (1 << 30) && q[1] == -(1 << 30), "2^30 exactly must be accepted");
        CHECK(!sn::torus_pose_q(k256, mw, mh, past, q), "the next double above 2^30 must be refused");
      }
      for (double bad : {nan, inf, -inf}) {
        check_pose(k256, mw, mh, bad, 1.0, 0.0);
        check_pose(k256, mw, mh, 1.0, bad, 0.0);
        check_pose(k256, mw, mh, 1.0, 1.0, bad);
        int32_t q[6];
        const double px[3] = {bad, 1.0, 0.0}, py[3] = {1.0, bad, 0.0}, pyaw[3] = {1.0, 1.0, bad};
        CHECK(!sn::torus_pose_q(k256, mw, mh, px, q) && !sn::torus_pose_q(k256, mw, mh, py, q) && !sn::torus_pose_q(k256, mw, mh, pyaw, q),
              "a field that is not finite must be refused");
      }
      // negative coordinates: tx >> 8 floors (-1 sub is cell -1, -256 subs is cell -1, -257 subs is cell -2)
      for (double subs : {-1.0, -128.0, -255.0, -256.0, -257.0, -511.5, -512.0, 0.0, 255.0, 256.0, 0.5, 1.5, -0.5, -1.5, 2.5})
        check_pose(k256, mw, mh, subs / k256, -subs / k256, 3.0);
      if (k256 == 256.0) {
        int32_t q[6];
        const double p[3] = {-1.0 / 256.0, -257.0 / 256.0, 0.0};
        CHECK(sn::torus_pose_q(k256, mw, mh, p, q) && q[4] == -1 - mw / 2 && q[5] == -2 - mh / 2, "the origin of a negative pose must floor");
      }
      uint64_t r = 0x9e3779b97f4a7c15ull;      // a sweep: xorshift, poses over +-2^30 subs and every yaw
      for (int it = 0; it < 2000; ++it) {
        double u[3];
        for (double& v : u) {
          r ^= r << 13, r ^= r >> 7, r ^= r << 17;
          v = (double)(r >> 11) / 9007199254740992.0 * 2.0 - 1.0;
        }
        check_pose(k256, mw, mh, u[0] * std::ldexp(1.0, it % 31) / k256, u[1] * std::ldexp(1.0, 30 - it % 31) / k256, u[2] * 7.0);
      }
    }
}

}  // namespace

int main() {
  check_grouper();
  check_pose_rule();
  if (failures) {
    std::fprintf(stderr, "stream_groups_check: %d failures\n", failures);
    return 1;
  }
  std::printf("stream_groups_check: ok\n");
  return 0;
}
