// pointcloud_harness.cpp — drives StereonetNode through the in-process rclcpp stand-in like node_harness, and records both
// the disparity message and the sensor_msgs/PointCloud2 of /stereonet_pointcloud2 (STEREONET_POINTCLOUD set).
//   pointcloud_harness <model.snw> <sbs_nv12.bin> <w> <h> <nframes> <out_prefix>
// writes <out_prefix>.<i>.msg (disparity payload) and <out_prefix>.<i>.pc (cloud data bytes), and prints one line per
// message: "frame_id=... len=..." for the disparity topic, "cloud frame_id=... stamp=... height=... width=...
// point_step=... row_step=... is_dense=... is_bigendian=... fields=name:offset:datatype:count,... len=..." for the cloud.
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
  int received = 0, clouds = 0;
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
  auto sub_pc = listener.create_subscription<sensor_msgs::msg::PointCloud2>(
      "stereonet_pointcloud2", 10, [&](sensor_msgs::msg::PointCloud2::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(prefix + "." + std::to_string(clouds) + ".pc", std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        std::string fields;
        for (const auto& f : m->fields)
          fields += (fields.empty() ? "" : ",") + f.name + ":" + std::to_string(f.offset) + ":" + std::to_string(f.datatype) +
                    ":" + std::to_string(f.count);
        printf("cloud frame_id=%s stamp=%d.%u height=%u width=%u point_step=%u row_step=%u is_dense=%d is_bigendian=%d "
               "fields=%s len=%zu\n",
               m->header.frame_id.c_str(), m->header.stamp.sec, m->header.stamp.nanosec, m->height, m->width, m->point_step,
               m->row_step, (int)m->is_dense, (int)m->is_bigendian, fields.c_str(), m->data.size());
        ++clouds;
        cv.notify_all();
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
    pub->publish(m);
  }
  {
    std::unique_lock<std::mutex> lk(mu);
    if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return received >= nframes; })) {
      fprintf(stderr, "timeout: %d messages, %d clouds of %d frames\n", received, clouds, nframes);
      return 4;
    }
  }
  // a frame's cloud is published by the same PostProcess call right after its disparity message: once the node is idle
  // every cloud it was going to publish has arrived
  node->WaitIdle();
  {
    std::lock_guard<std::mutex> lk(mu);
    printf("received=%d clouds=%d\n", received, clouds);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
