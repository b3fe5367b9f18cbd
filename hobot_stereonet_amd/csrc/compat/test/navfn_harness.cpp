// navfn_harness.cpp — inflate_harness with one more listener and a goal: drives StereonetNode through the in-process rclcpp
// stand-in, sets the base pose and the goal before every frame (StereonetNode::SetBasePose, SetGoal) and waits for the frame to
// leave the node before the next, and records the nav_msgs/OccupancyGrid of /stereonet_obstacle_grid, /stereonet_costmap
// (STEREONET_COSTMAP set) and /stereonet_inflated_grid (STEREONET_INFLATE set) and the nav_msgs/Path of /stereonet_plan
// (STEREONET_PLAN set).
//   navfn_harness <model.snw> <sbs_nv12.bin> <w> <h> <nframes> <out_prefix> <goal_x_m> <goal_y_m> [<poses.txt>]
// goal_x_m = "none": SetGoal is never called.  poses.txt: one `x y yaw` line per frame (missing: SetBasePose is never called).
// writes <out_prefix>.<i>.grid, .costmap and .inflated (the int8 data) and <out_prefix>.<i>.plan (the poses' x and y as float64
// pairs), and prints one line per message: "grid|costmap|inflated seq=... frame_id=... stamp=... width=... height=...
// resolution=... origin=x,y len=..." and "plan seq=... frame_id=... stamp=... poses=... pose_frames_ok=0|1" (floats as %.9g;
// seq counts every message of the four topics in the order of arrival).
// Exit code 3 = Init failed, 4 = timeout (disparity messages missing).
//
//   navfn_harness --bench <cost.bin> <gw> <gh> <goal_x> <goal_y> <neutral> <lethal_cost> <unknown_cost> <iters>
// the thing sn_navfn replaces, for scripts/bench_navfn.py: a plain binary-heap Dijkstra of the header's field on one host
// thread over the uint8 costs of cost.bin (unknown_cost -1: unknown cells are blocked); prints {"dijkstra_us": mean of iters runs, "reached": cells,
// "checksum": the sum of the finite words modulo 2^64}.
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "stereonet_node.h"

using hobot::stereonet::StereonetNode;

namespace {

// P of the header over one map -> the cells reached
size_t dijkstra(const std::vector<uint8_t>& cost, int gw, int gh, int gx, int gy, int neutral, int lethal, int unknown,
                std::vector<uint32_t>* pot) {
  static const int dx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, dy[8] = {0, -1, -1, -1, 0, 1, 1, 1};
  std::vector<uint16_t> w((size_t)gw * gh);
  for (size_t i = 0; i < w.size(); ++i) w[i] = cost[i] == 255 ? (unknown < 0 ? 0 : (uint16_t)(neutral + unknown)) : cost[i] >= lethal ? 0 : (uint16_t)(neutral + cost[i]);
  pot->assign(w.size(), SN_NAV_INF);
  if (gx < 0 || gx >= gw || gy < 0 || gy >= gh || !w[(size_t)gy * gw + gx]) return 0;
  using Item = std::pair<uint32_t, int>;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  (*pot)[(size_t)gy * gw + gx] = 0;
  heap.push({0u, gy * gw + gx});
  size_t reached = 0;
  while (!heap.empty()) {
    const Item top = heap.top();
    heap.pop();
    if (top.first != (*pot)[top.second]) continue;
    ++reached;
    const int ay = top.second / gw, ax = top.second - ay * gw;
    for (int d = 0; d < 8; ++d) {
      const int bx = ax + dx[d], by = ay + dy[d];
      if (bx < 0 || bx >= gw || by < 0 || by >= gh) continue;
      const int b = by * gw + bx;
      if (!w[b] || ((d & 1) && (!w[ay * gw + bx] || !w[by * gw + ax]))) continue;
      const uint32_t cand = top.first + (uint32_t)((d & 1) ? 7 : 5) * w[b];
      if (cand < (*pot)[b]) {
        (*pot)[b] = cand;
        heap.push({cand, b});
      }
    }
  }
  return reached;
}

int bench(int argc, char** argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: %s --bench cost.bin gw gh goal_x goal_y neutral lethal_cost unknown_cost iters\n", argv[0]);
    return 2;
  }
  const int gw = atoi(argv[3]), gh = atoi(argv[4]), gx = atoi(argv[5]), gy = atoi(argv[6]), neutral = atoi(argv[7]), lethal = atoi(argv[8]);
  const int unknown = atoi(argv[9]), iters = atoi(argv[10]);
  if (gw < 1 || gh < 1 || gw > 4096 || gh > 4096 || iters < 1) return 2;
  std::vector<uint8_t> cost((size_t)gw * gh);
  std::ifstream f(argv[2], std::ios::binary);
  f.read(reinterpret_cast<char*>(cost.data()), cost.size());
  if ((size_t)f.gcount() != cost.size()) return 2;
  std::vector<uint32_t> pot;
  size_t reached = dijkstra(cost, gw, gh, gx, gy, neutral, lethal, unknown, &pot);      // warm
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < iters; ++i) reached = dijkstra(cost, gw, gh, gx, gy, neutral, lethal, unknown, &pot);
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / iters;
  unsigned long long sum = 0;
  for (uint32_t v : pot)
    if (v != SN_NAV_INF) sum += v;
  printf("{\"dijkstra_us\": %.3f, \"reached\": %zu, \"checksum\": %llu}\n", us, reached, sum);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--bench")) return bench(argc, argv);
  if (argc < 9) {
    fprintf(stderr, "usage: %s model sbs.bin w h nframes out_prefix goal_x_m|none goal_y_m [poses.txt]\n", argv[0]);
    return 2;
  }
  const std::string model = argv[1], sbs_path = argv[2], prefix = argv[6];
  const int w = atoi(argv[3]), h = atoi(argv[4]), nframes = atoi(argv[5]);
  const bool with_goal = strcmp(argv[7], "none") != 0;
  const double goal_x = atof(argv[7]), goal_y = atof(argv[8]);
  rclcpp::init(argc, argv);
  rclcpp::NodeOptions opt;
  opt.append_parameter_override("model_file", model);
  auto node = std::make_shared<StereonetNode>("stereonet_node", opt);
  if (!rclcpp::ok() || !node->IsReady()) {
    fprintf(stderr, "node init failed\n");
    return 3;
  }
  std::vector<uint8_t> sbs((size_t)2 * w * h * 3 / 2);
  {
    std::ifstream f(sbs_path, std::ios::binary);
    f.read(reinterpret_cast<char*>(sbs.data()), sbs.size());
    if ((size_t)f.gcount() != sbs.size()) return 2;
  }
  std::mutex mu;
  std::condition_variable cv;
  int received = 0, grids = 0, maps = 0, inflated = 0, plans = 0, seq = 0;
  std::vector<double> poses;
  if (argc > 9) {
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
    printf("%s seq=%d frame_id=%s stamp=%d.%u width=%u height=%u resolution=%.9g origin=%.9g,%.9g len=%zu\n", kind, seq, m.header.frame_id.c_str(),
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
    std::ofstream o(prefix + "." + std::to_string(plans) + ".plan", std::ios::binary);
    bool same = true;
    for (const auto& ps : m->poses) {
      const double xy[2] = {ps.pose.position.x, ps.pose.position.y};
      o.write(reinterpret_cast<const char*>(xy), sizeof(xy));
      same = same && ps.header.frame_id == m->header.frame_id && ps.header.stamp.sec == m->header.stamp.sec &&
             ps.header.stamp.nanosec == m->header.stamp.nanosec;
    }
    printf("plan seq=%d frame_id=%s stamp=%d.%u poses=%zu pose_frames_ok=%d\n", seq, m->header.frame_id.c_str(), m->header.stamp.sec,
           m->header.stamp.nanosec, m->poses.size(), same ? 1 : 0);
    ++plans, ++seq;
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
    pub->publish(m);
    // one frame at a time: the pose set above is this frame's, and the next is set only after this frame has left the node
    std::unique_lock<std::mutex> lk(mu);
    if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return received > i; })) {
      fprintf(stderr, "timeout: %d messages, %d grids, %d maps, %d plans of %d frames\n", received, grids, maps, plans, nframes);
      return 4;
    }
    lk.unlock();
    // a frame's grids and plan are published by the same PostProcess call right after its disparity message: once the node is
    // idle everything it was going to publish has arrived
    node->WaitIdle();
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    printf("received=%d grids=%d maps=%d inflated=%d plans=%d\n", received, grids, maps, inflated, plans);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
