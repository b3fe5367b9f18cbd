// elevation_harness.cpp — drives StereonetNode through the in-process rclcpp stand-in like costmap_harness, sets the base pose
// before every frame (StereonetNode::SetBasePose) and waits for the frame to leave the node before the next, and records the
// disparity message, the nav_msgs/OccupancyGrid of /stereonet_traversability (STEREONET_ELEVATION set) and that of
// /stereonet_inflated_grid (STEREONET_INFLATE set; its source is the traversability grid when the elevation file says
// `feed_inflate 1`).  A stand-alone program: it can be built with a sanitizer on the host code and run as it is.
//   elevation_harness <model.snw> <sbs_nv12.bin> <w> <h> <nframes> <out_prefix> [<poses.txt>]
// poses.txt: one `x y yaw` line per frame (missing: SetBasePose is never called).
// writes <out_prefix>.<i>.msg (disparity payload), <out_prefix>.<i>.trav (the verdict's int8 data) and <out_prefix>.<i>.inflated
// (the inflated grid's int8 data), and prints one line per message: "frame_id=... len=..." for the disparity topic and
// "traversability seq=... frame_id=... stamp=... width=... height=... resolution=... origin=x,y len=... known=... lethal=..." and
// "inflated seq=... frame_id=... stamp=... width=... height=... resolution=... origin=x,y len=..." (floats as %.9g; seq counts
// every message of the two grid topics in the order of arrival).
// Exit code 3 = Init failed, 4 = timeout (disparity messages missing).
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>

#include "stereonet_node.h"

using hobot::stereonet::StereonetNode;

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s model sbs.bin w h nframes out_prefix\n", argv[0]);
    return 2;
  }
  const std::string model = argv[1], sbs_path = argv[2], prefix = argv[6];
  const int w = atoi(argv[3]), h = atoi(argv[4]), nframes = atoi(argv[5]);
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
  int received = 0, travs = 0, inflated = 0, seq = 0;
  std::vector<double> poses;
  if (argc > 7) {
    std::ifstream f(argv[7]);
    double v;
    while (f >> v) poses.push_back(v);
  }
  rclcpp::Node listener("listener");
  auto sub = listener.create_subscription<sensor_msgs::msg::Image>(
      "stereonet_node_output", 10, [&](sensor_msgs::msg::Image::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(prefix + "." + std::to_string(received) + ".msg", std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        printf("frame_id=%s len=%zu\n", m->header.frame_id.c_str(), m->data.size());
        ++received;
        cv.notify_all();
      });
  auto sub_trav = listener.create_subscription<nav_msgs::msg::OccupancyGrid>(
      "stereonet_traversability", 10, [&](nav_msgs::msg::OccupancyGrid::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(prefix + "." + std::to_string(travs) + ".trav", std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        size_t known = 0, lethal = 0;
        for (int8_t v : m->data) known += v >= 0, lethal += v == 100;
        printf("traversability seq=%d frame_id=%s stamp=%d.%u width=%u height=%u resolution=%.9g origin=%.9g,%.9g len=%zu known=%zu lethal=%zu\n",
               seq, m->header.frame_id.c_str(), m->header.stamp.sec, m->header.stamp.nanosec, m->info.width, m->info.height,
               m->info.resolution, m->info.origin.position.x, m->info.origin.position.y, m->data.size(), known, lethal);
        ++travs, ++seq;
      });
  auto sub_inflated = listener.create_subscription<nav_msgs::msg::OccupancyGrid>(
      "stereonet_inflated_grid", 10, [&](nav_msgs::msg::OccupancyGrid::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(prefix + "." + std::to_string(inflated) + ".inflated", std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        printf("inflated seq=%d frame_id=%s stamp=%d.%u width=%u height=%u resolution=%.9g origin=%.9g,%.9g len=%zu\n", seq,
               m->header.frame_id.c_str(), m->header.stamp.sec, m->header.stamp.nanosec, m->info.width, m->info.height,
               m->info.resolution, m->info.origin.position.x, m->info.origin.position.y, m->data.size());
        ++inflated, ++seq;
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
    pub->publish(m);
    // one frame at a time: the pose set above is this frame's, and the next is set only after this frame has left the node
    std::unique_lock<std::mutex> lk(mu);
    if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return received > i; })) {
      fprintf(stderr, "timeout: %d messages, %d traversability grids, %d inflated grids of %d frames\n", received, travs, inflated, nframes);
      return 4;
    }
    lk.unlock();
    // a frame's grids are published by the same PostProcess call right after its disparity message: once the node is idle
    // everything it was going to publish has arrived
    node->WaitIdle();
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    printf("received=%d traversability=%d inflated=%d\n", received, travs, inflated);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
