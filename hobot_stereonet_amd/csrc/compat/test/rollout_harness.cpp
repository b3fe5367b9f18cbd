// rollout_harness <model.snw> <sbs_nv12.bin> <w> <h> <nframes> <out_prefix> <goal_x_m|none> <goal_y_m> <poses.txt|none> [<v> <w>]
// Starts a StereonetNode with whatever STEREONET_* the caller exported (the obstacle grid, optionally the costmap, the
// inflation, the plan and the rollout: STEREONET_ROLLOUT), sets the goal and, when given, the velocity, publishes the same
// side-by-side NV12 frame nframes times with line k of poses.txt as SetBasePose, and records what arrives on
// /stereonet_obstacle_grid, /stereonet_costmap and /stereonet_inflated_grid (data to <out_prefix>.<k>.grid / .costmap /
// .inflated), /stereonet_plan, /stereonet_cmd_vel and /stereonet_local_plan (<out_prefix>.<k>.local_plan: x, y, qz, qw as
// doubles per pose).  One line per message in the order of arrival:
//   cmd seq=<n> v=<linear.x> w=<angular.z> rest=<the sum of the other four components>
//   local_plan seq=<n> frame_id=... stamp=... poses=<n> pose_frames_ok=<0|1>
// Exit code 3 = Init failed, 4 = timeout (disparity messages missing).
//
//   rollout_harness --bench <cost.bin> <potential.bin> <centres.bin> <offsets.bin> <gw> <gh> <nv> <nw> <steps> <nf>
//                   <px> <py> <cq> <sq> <lethal_cost> <centre_lethal_cost> <unknown_cost> <w_goal> <w_occ> <iters>
// the thing sn_rollout replaces: a plain loop on one host thread over the library's own tables (centres int32 [S][T+1][3],
// offsets int32 [nw][T+1][nf][2], as sn_rollout_tables writes them), sample by sample, step by step, point by point, for one
// map; a sample leaves at its first collision, as a host planner would write it (unknown_cost -1: unknown cells collide).
// Prints {"loop_us": mean of iters runs, "s_best", "score", "valid", "collided", "no_route"}.
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>

#include "stereonet_node.h"

using hobot::stereonet::StereonetNode;

namespace {

template <class T>
bool read_all(const char* path, std::vector<T>* v) {
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(v->data()), v->size() * sizeof(T));
  return (size_t)f.gcount() == v->size() * sizeof(T);
}

struct Job {
  std::vector<uint8_t> cost;
  std::vector<uint32_t> pot;
  std::vector<int32_t> centres, offsets;
  int gw, gh, nv, nw, T, nf;
  long long px, py, cq, sq;
  int lethal, centre_lethal, unknown, w_goal, w_occ;
};

struct Result {
  unsigned long long key = ~0ull;
  int valid = 0, collided = 0, no_route = 0;
};

Result walk(const Job& j) {
  Result r;
  const int S = j.nv * j.nw, T1 = j.T + 1;
  for (int s = 0; s < S; ++s) {
    const int iw = s % j.nw;
    const int32_t* cen = j.centres.data() + (size_t)s * T1 * 3;
    int occ = 0;
    bool hit = false;
    long long cx = 0, cy = 0;
    for (int t = 0; t < T1 && !hit; ++t) {
      const int32_t* off = j.offsets.data() + ((size_t)iw * T1 + t) * j.nf * 2;
      for (int f = 0; f <= j.nf && !hit; ++f) {
        long long qx = cen[3 * t], qy = cen[3 * t + 1];
        if (f) qx += off[2 * (f - 1)], qy += off[2 * (f - 1) + 1];
        cx = (j.px + ((j.cq * qx - j.sq * qy + (1ll << 29)) >> 30)) >> 8;
        cy = (j.py + ((j.sq * qx + j.cq * qy + (1ll << 29)) >> 30)) >> 8;
        if (cx < 0 || cx >= j.gw || cy < 0 || cy >= j.gh) {
          hit = true;
          break;
        }
        const int c = j.cost[(size_t)cy * j.gw + cx];
        if (c == 255) {
          if (j.unknown < 0) hit = true;
          else if (j.unknown > occ) occ = j.unknown;
        } else if (c >= (f ? j.lethal : j.centre_lethal)) {
          hit = true;
        } else if (c > occ) {
          occ = c;
        }
      }
    }
    if (hit) {
      ++r.collided;
      continue;
    }
    const int32_t* last = cen + 3 * j.T;
    cx = (j.px + ((j.cq * last[0] - j.sq * last[1] + (1ll << 29)) >> 30)) >> 8;
    cy = (j.py + ((j.sq * last[0] + j.cq * last[1] + (1ll << 29)) >> 30)) >> 8;
    const uint32_t g = j.pot[(size_t)cy * j.gw + cx];
    if (g == SN_NAV_INF) {
      ++r.no_route;
      continue;
    }
    ++r.valid;
    const unsigned long long key = ((unsigned long long)j.w_goal * g + (unsigned long long)j.w_occ * occ) << 16 | (unsigned)s;
    if (key < r.key) r.key = key;
  }
  return r;
}

int bench(int argc, char** argv) {
  if (argc < 22) {
    fprintf(stderr, "usage: %s --bench cost.bin potential.bin centres.bin offsets.bin gw gh nv nw steps nf px py cq sq lethal_cost "
                    "centre_lethal_cost unknown_cost w_goal w_occ iters\n", argv[0]);
    return 2;
  }
  Job j;
  j.gw = atoi(argv[6]), j.gh = atoi(argv[7]), j.nv = atoi(argv[8]), j.nw = atoi(argv[9]), j.T = atoi(argv[10]), j.nf = atoi(argv[11]);
  j.px = atoll(argv[12]), j.py = atoll(argv[13]), j.cq = atoll(argv[14]), j.sq = atoll(argv[15]);
  j.lethal = atoi(argv[16]), j.centre_lethal = atoi(argv[17]), j.unknown = atoi(argv[18]), j.w_goal = atoi(argv[19]), j.w_occ = atoi(argv[20]);
  const int iters = atoi(argv[21]);
  if (j.gw < 1 || j.gh < 1 || j.gw > 4096 || j.gh > 4096 || j.nv < 1 || j.nv > 64 || j.nw < 1 || j.nw > 64 || j.T < 1 ||
      j.T > SN_ROLLOUT_MAX_STEPS || j.nf < 0 || j.nf > SN_ROLLOUT_MAX_POINTS || iters < 1)
    return 2;
  j.cost.resize((size_t)j.gw * j.gh), j.pot.resize(j.cost.size());
  j.centres.resize((size_t)j.nv * j.nw * (j.T + 1) * 3), j.offsets.resize((size_t)j.nw * (j.T + 1) * j.nf * 2);
  if (!read_all(argv[2], &j.cost) || !read_all(argv[3], &j.pot) || !read_all(argv[4], &j.centres) || !read_all(argv[5], &j.offsets)) return 2;
  Result r = walk(j);      // warm
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) r = walk(j);
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / iters;
  const bool none = r.key == ~0ull;
  printf("{\"loop_us\": %.3f, \"s_best\": %lld, \"score\": %lld, \"valid\": %d, \"collided\": %d, \"no_route\": %d}\n", us,
         none ? -1ll : (long long)(r.key & 0xFFFF), none ? -1ll : (long long)(r.key >> 16), r.valid, r.collided, r.no_route);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--bench")) return bench(argc, argv);
  if (argc < 10) {
    fprintf(stderr, "usage: %s model sbs.bin w h nframes out_prefix goal_x_m|none goal_y_m poses.txt|none [v w]\n       %s --bench ...\n", argv[0], argv[0]);
    return 2;
  }
  const std::string model = argv[1], sbs_path = argv[2], prefix = argv[6];
  const int w = atoi(argv[3]), h = atoi(argv[4]), nframes = atoi(argv[5]);
  const bool with_goal = strcmp(argv[7], "none") != 0, with_velocity = argc > 11;
  const double goal_x = atof(argv[7]), goal_y = atof(argv[8]);
  const double vel_v = with_velocity ? atof(argv[10]) : 0.0, vel_w = with_velocity ? atof(argv[11]) : 0.0;
  rclcpp::init(argc, argv);
  rclcpp::NodeOptions opt;
  opt.append_parameter_override("model_file", model);
  auto node = std::make_shared<StereonetNode>("stereonet_node", opt);
  if (!rclcpp::ok() || !node->IsReady()) {
    fprintf(stderr, "node init failed\n");
    return 3;
  }
  std::vector<uint8_t> sbs((size_t)2 * w * h * 3 / 2);
  if (!read_all(sbs_path.c_str(), &sbs)) return 2;
  std::mutex mu;
  std::condition_variable cv;
  int received = 0, grids = 0, maps = 0, inflated = 0, plans = 0, cmds = 0, arcs = 0, seq = 0;
  std::vector<double> poses;
  if (strcmp(argv[9], "none") != 0) {
    std::ifstream f(argv[9]);
    double v;
    while (f >> v) poses.push_back(v);
  }
  rclcpp::Node listener("listener");
  auto sub = listener.create_subscription<sensor_msgs::msg::Image>("stereonet_node_output", 10, [&](sensor_msgs::msg::Image::ConstSharedPtr) {
    std::lock_guard<std::mutex> lk(mu);
    ++received;
    cv.notify_all();
  });
  auto record = [&](const char* kind, int* count, const nav_msgs::msg::OccupancyGrid& m) {
    std::lock_guard<std::mutex> lk(mu);
    std::ofstream o(prefix + "." + std::to_string(*count) + "." + kind, std::ios::binary);
    o.write(reinterpret_cast<const char*>(m.data.data()), m.data.size());
    printf("%s seq=%d frame_id=%s stamp=%d.%u width=%u height=%u resolution=%.9g origin=%.17g,%.17g len=%zu\n", kind, seq, m.header.frame_id.c_str(),
           m.header.stamp.sec, m.header.stamp.nanosec, m.info.width, m.info.height, m.info.resolution, m.info.origin.position.x,
           m.info.origin.position.y, m.data.size());
    ++*count, ++seq;
  };
  auto sub_grid = listener.create_subscription<nav_msgs::msg::OccupancyGrid>(
      "stereonet_obstacle_grid", 10, [&](nav_msgs::msg::OccupancyGrid::ConstSharedPtr m) { record("grid", &grids, *m); });
  auto sub_map = listener.create_subscription<nav_msgs::msg::OccupancyGrid>(
      "stereonet_costmap", 10, [&](nav_msgs::msg::OccupancyGrid::ConstSharedPtr m) { record("costmap", &maps, *m); });
  auto sub_inflated = listener.create_subscription<nav_msgs::msg::OccupancyGrid>(
      "stereonet_inflated_grid", 10, [&](nav_msgs::msg::OccupancyGrid::ConstSharedPtr m) { record("inflated", &inflated, *m); });
  auto sub_plan = listener.create_subscription<nav_msgs::msg::Path>("stereonet_plan", 10, [&](nav_msgs::msg::Path::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    printf("plan seq=%d frame_id=%s stamp=%d.%u poses=%zu\n", seq, m->header.frame_id.c_str(), m->header.stamp.sec, m->header.stamp.nanosec,
           m->poses.size());
    ++plans, ++seq;
  });
  auto sub_cmd = listener.create_subscription<geometry_msgs::msg::Twist>("stereonet_cmd_vel", 10, [&](geometry_msgs::msg::Twist::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    printf("cmd seq=%d v=%.17g w=%.17g rest=%.17g\n", seq, m->linear.x, m->angular.z, m->linear.y + m->linear.z + m->angular.x + m->angular.y);
    ++cmds, ++seq;
  });
  auto sub_arc = listener.create_subscription<nav_msgs::msg::Path>("stereonet_local_plan", 10, [&](nav_msgs::msg::Path::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    std::ofstream o(prefix + "." + std::to_string(arcs) + ".local_plan", std::ios::binary);
    bool same = true;
    for (const auto& ps : m->poses) {
      const double v[4] = {ps.pose.position.x, ps.pose.position.y, ps.pose.orientation.z, ps.pose.orientation.w};
      o.write(reinterpret_cast<const char*>(v), sizeof(v));
      same = same && ps.header.frame_id == m->header.frame_id && ps.header.stamp.sec == m->header.stamp.sec &&
             ps.header.stamp.nanosec == m->header.stamp.nanosec && ps.pose.position.z == 0.0 && ps.pose.orientation.x == 0.0 &&
             ps.pose.orientation.y == 0.0;
    }
    printf("local_plan seq=%d frame_id=%s stamp=%d.%u poses=%zu pose_frames_ok=%d\n", seq, m->header.frame_id.c_str(), m->header.stamp.sec,
           m->header.stamp.nanosec, m->poses.size(), same ? 1 : 0);
    ++arcs, ++seq;
  });
  auto pub = listener.create_publisher<hbm_img_msgs::msg::HbmMsg1080P>("hbmem_stereo_img", 10);
  for (int i = 0; i < nframes; ++i) {
    hbm_img_msgs::msg::HbmMsg1080P m;
    m.index = 100 + i;
    m.time_stamp.sec = 7;
    m.time_stamp.nanosec = 1000 + i;
    m.height = h;
    m.width = 2 * w;
    m.data_size = (uint32_t)sbs.size();
    memcpy(m.encoding.data(), "nv12", 5);
    m.data = sbs;
    for (size_t k = 0; k < (size_t)w; k += 7) m.data[k] ^= (uint8_t)(i * 5);   // frames differ (luma of the first row)
    if ((size_t)(3 * i + 2) < poses.size()) node->SetBasePose(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2]);
    if (with_goal) node->SetGoal(goal_x, goal_y);
    if (with_velocity) node->SetVelocity(vel_v, vel_w);
    pub->publish(m);
    // one frame at a time: the pose set above is this frame's, and the next is set only after this frame has left the node
    std::unique_lock<std::mutex> lk(mu);
    if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return received > i; })) {
      fprintf(stderr, "timeout: %d messages, %d plans, %d commands of %d frames\n", received, plans, cmds, nframes);
      return 4;
    }
    lk.unlock();
    node->WaitIdle();      // everything the frame's PostProcess publishes has arrived once the node is idle
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    printf("received=%d grids=%d maps=%d inflated=%d plans=%d cmds=%d local_plans=%d\n", received, grids, maps, inflated, plans, cmds, arcs);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
