// render_harness.cpp — drives StereonetNode through the in-process rclcpp stand-in like temporal_harness, with a file of
// several different side-by-side NV12 frames, and records the disparity messages and what the node publishes on /image_jpeg.
// Whether it publishes there is decided by STEREONET_RENDER.
//   render_harness <model.snw> <frames.bin> <w> <h> <nframes> <out_prefix>
// frames.bin holds nframes frames of 2w * h * 3 / 2 bytes each, published in file order; writes <out_prefix>.<i>.msg (payload
// bytes: the int32 tensor, then the JPEG of the left eye) and, per /image_jpeg message, <out_prefix>.<j>.render.jpg (its data)
// and <out_prefix>.<j>.render.txt ("frame_id width height step encoding"); prints "received=N rendered=M" at the end.
// Exit code 2 = usage / short file, 3 = Init failed, 4 = timeout.
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
    fprintf(stderr, "usage: %s model frames.bin w h nframes out_prefix\n", argv[0]);
    return 2;
  }
  const std::string model = argv[1], frames_path = argv[2], prefix = argv[6];
  const int w = atoi(argv[3]), h = atoi(argv[4]), nframes = atoi(argv[5]);
  if (w <= 0 || h <= 0 || nframes <= 0) return 2;
  const size_t frame_bytes = (size_t)2 * w * h * 3 / 2;
  std::vector<uint8_t> frames(frame_bytes * nframes);
  {
    std::ifstream f(frames_path, std::ios::binary);
    f.read(reinterpret_cast<char*>(frames.data()), frames.size());
    if ((size_t)f.gcount() != frames.size()) {
      fprintf(stderr, "%s holds fewer than %d frames of %zu bytes\n", frames_path.c_str(), nframes, frame_bytes);
      return 2;
    }
  }
  rclcpp::init(argc, argv);
  rclcpp::NodeOptions opt;
  opt.append_parameter_override("model_file", model);
  auto node = std::make_shared<StereonetNode>("stereonet_node", opt);
  if (!rclcpp::ok() || !node->IsReady()) {
    fprintf(stderr, "node init failed\n");
    return 3;
  }
  std::mutex mu;
  std::condition_variable cv;
  int received = 0, rendered = 0;
  rclcpp::Node listener("listener");
  auto view = listener.create_subscription<sensor_msgs::msg::Image>("/image_jpeg", 10, [&](sensor_msgs::msg::Image::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    const std::string base = prefix + "." + std::to_string(rendered) + ".render";
    std::ofstream o(base + ".jpg", std::ios::binary);
    o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
    std::ofstream t(base + ".txt");
    t << m->header.frame_id << " " << m->width << " " << m->height << " " << m->step << " " << m->encoding << "\n";
    ++rendered;
    cv.notify_all();
  });
  auto sub = listener.create_subscription<sensor_msgs::msg::Image>(
      "stereonet_node_output", 10, [&](sensor_msgs::msg::Image::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(prefix + "." + std::to_string(received) + ".msg", std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        printf("frame_id=%s len=%zu\n", m->header.frame_id.c_str(), m->data.size());
        ++received;
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
    m.data_size = (uint32_t)frame_bytes;
    memcpy(m.encoding.data(), "nv12", 5);
    m.data.assign(frames.begin() + (size_t)i * frame_bytes, frames.begin() + (size_t)(i + 1) * frame_bytes);
    pub->publish(m);
  }
  {
    std::unique_lock<std::mutex> lk(mu);
    if (!cv.wait_for(lk, std::chrono::seconds(60), [&] { return received >= nframes; })) {
      fprintf(stderr, "timeout: %d of %d frames\n", received, nframes);
      return 4;
    }
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    printf("received=%d rendered=%d\n", received, rendered);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
