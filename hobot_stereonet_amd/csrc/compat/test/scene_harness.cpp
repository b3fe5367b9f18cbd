// scene_harness <model.snw> <w> <h> <raws.bin> <nframes> <poses.txt> <goal_x> <goal_y> <out_prefix> [<v> <w>]
// Starts a StereonetNode with whatever STEREONET_* the caller exported and hands its PostProcess prepared requests: frame k's
// output tensor is map k of raws.bin (int32 [nframes][h][w], the model's size), so the scene the node publishes about is the
// caller's and not what a network made of a picture.  No inference runs and no input frame is published; the model file only
// gives the engine its geometry.  Per frame, in this order: SetBasePose(line k of poses.txt: x y yaw), SetGoal, SetVelocity when
// given, the request (header stamp 7.(1000 + k), frame id "100 + k", a flat grey side-by-side frame, rt_stat as Run leaves it),
// WaitIdle.  Every message on /stereonet_obstacle_grid, /stereonet_scan, /stereonet_costmap, /stereonet_inflated_grid,
// /stereonet_plan, /stereonet_cmd_vel, /stereonet_local_plan and /stereonet_pointcloud2 is recorded whole: one line per
// message on stdout in the order of arrival, `<kind> seq=<n> key=value ...`, with its arrays in <out_prefix>.<seq>.<kind>:
//   grid | costmap | inflated   frame_id stamp load resolution width height origin=px,py,pz,qx,qy,qz,qw; the file is data, int8
//   scan                        frame_id stamp angle_min angle_max angle_increment time_increment scan_time range_min range_max
//                               ranges intensities (counts); the file is ranges, float32
//   plan | local_plan           frame_id stamp poses; the file is text, a line per pose: frame_id sec nanosec x y z qx qy qz qw
//   cmd                         lx ly lz ax ay az
//   cloud                       frame_id stamp height width point_step row_step is_dense is_bigendian
//                               fields=name:offset:datatype:count,...; the file is data
// Exit code 3 = Init failed, 4 = timeout (a frame did not leave the node within 60 s).
#include <unistd.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <mutex>
#include <string>
#include <vector>

#include "stereonet_node.h"

using hobot::stereonet::StereonetNode;
using hobot::stereonet::StereonetNodeOutput;

namespace {

// the one thing the node does not offer from outside: PostProcess on a request whose tensor is the caller's map
class SceneNode : public StereonetNode {
 public:
  using StereonetNode::StereonetNode;
  int Inject(const int32_t* raw, int w, int h, int k) {
    auto request = std::make_shared<StereonetNodeOutput>();
    request->msg_header = std::make_shared<std_msgs::msg::Header>();
    request->msg_header->frame_id = std::to_string(100 + k);
    request->msg_header->stamp.sec = 7;
    request->msg_header->stamp.nanosec = 1000 + k;
    map_.assign(raw, raw + (size_t)w * h);      // a stage may filter the tensor in place
    auto tensor = std::make_shared<hobot::dnn_node::DNNTensor>();
    tensor->sysMem[0].virAddr = map_.data();
    tensor->sysMem[0].memSize = (uint32_t)(map_.size() * sizeof(int32_t));
    request->output_tensors.push_back(tensor);
    auto frame = std::make_shared<hbm_img_msgs::msg::HbmMsg1080P>();      // grey: luma and chroma at 128
    frame->index = 100 + k;
    frame->time_stamp = request->msg_header->stamp;
    frame->height = h, frame->width = 2 * w;
    frame->data.assign((size_t)2 * w * (h + (h + 1) / 2), 128);
    frame->data_size = (uint32_t)frame->data.size();
    memcpy(frame->encoding.data(), "nv12", 5);
    request->frame = frame;
    auto left = std::make_shared<hobot::stereonet::BinDataType>();      // no JPEG: the disparity message is not what is under test
    left->w = w, left->h = h;
    request->sp_left_nv12 = left;
    request->rt_stat = std::make_shared<hobot::dnn_node::DnnNodeRunTimeStat>();
    return PostProcess(request);
  }

 private:
  std::vector<int32_t> map_;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 10) {
    fprintf(stderr, "usage: %s model w h raws.bin nframes poses.txt goal_x_m goal_y_m out_prefix [v w]\n", argv[0]);
    return 2;
  }
  const std::string model = argv[1], prefix = argv[9];
  const int w = atoi(argv[2]), h = atoi(argv[3]), nframes = atoi(argv[5]);
  const double goal_x = atof(argv[7]), goal_y = atof(argv[8]);
  const bool with_velocity = argc > 11;
  const double vel_v = with_velocity ? atof(argv[10]) : 0.0, vel_w = with_velocity ? atof(argv[11]) : 0.0;
  if (w < 1 || h < 1 || nframes < 1) return 2;
  std::vector<int32_t> raws((size_t)nframes * w * h);
  {
    std::ifstream f(argv[4], std::ios::binary);
    f.read(reinterpret_cast<char*>(raws.data()), raws.size() * sizeof(int32_t));
    if ((size_t)f.gcount() != raws.size() * sizeof(int32_t)) return 2;
  }
  std::vector<double> poses;
  {
    std::ifstream f(argv[6]);
    double v;
    while (f >> v) poses.push_back(v);
    if (poses.size() < (size_t)3 * nframes) return 2;
  }
  rclcpp::init(argc, argv);
  rclcpp::NodeOptions opt;
  opt.append_parameter_override("model_file", model);
  auto node = std::make_shared<SceneNode>("stereonet_node", opt);
  if (!rclcpp::ok() || !node->IsReady()) {
    fprintf(stderr, "node init failed\n");
    return 3;
  }
  std::mutex mu;
  int seq = 0;
  auto file_of = [&](const char* kind) { return prefix + "." + std::to_string(seq) + "." + kind; };
  auto header = [](const std_msgs::msg::Header& hd) {
    char b[256];
    snprintf(b, sizeof(b), "frame_id=%s stamp=%d.%u", hd.frame_id.c_str(), hd.stamp.sec, hd.stamp.nanosec);
    return std::string(b);
  };
  auto grid = [&](const char* kind, const nav_msgs::msg::OccupancyGrid& m) {
    std::lock_guard<std::mutex> lk(mu);
    std::ofstream o(file_of(kind), std::ios::binary);
    o.write(reinterpret_cast<const char*>(m.data.data()), m.data.size());
    const auto& p = m.info.origin;
    printf("%s seq=%d %s load=%d.%u resolution=%.9g width=%u height=%u origin=%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g len=%zu\n", kind, seq,
           header(m.header).c_str(), m.info.map_load_time.sec, m.info.map_load_time.nanosec, m.info.resolution, m.info.width, m.info.height,
           p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w, m.data.size());
    ++seq;
  };
  auto path = [&](const char* kind, const nav_msgs::msg::Path& m) {
    std::lock_guard<std::mutex> lk(mu);
    FILE* o = fopen(file_of(kind).c_str(), "w");
    for (const auto& ps : m.poses) {
      const auto& p = ps.pose;
      if (o)
        fprintf(o, "%s %d %u %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", ps.header.frame_id.c_str(), ps.header.stamp.sec, ps.header.stamp.nanosec,
                p.position.x, p.position.y, p.position.z, p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w);
    }
    if (o) fclose(o);
    printf("%s seq=%d %s poses=%zu\n", kind, seq, header(m.header).c_str(), m.poses.size());
    ++seq;
  };
  rclcpp::Node listener("listener");
  using Grid = nav_msgs::msg::OccupancyGrid;
  auto sub_grid = listener.create_subscription<Grid>("stereonet_obstacle_grid", 10, [&](Grid::ConstSharedPtr m) { grid("grid", *m); });
  auto sub_map = listener.create_subscription<Grid>("stereonet_costmap", 10, [&](Grid::ConstSharedPtr m) { grid("costmap", *m); });
  auto sub_inflated = listener.create_subscription<Grid>("stereonet_inflated_grid", 10, [&](Grid::ConstSharedPtr m) { grid("inflated", *m); });
  auto sub_plan = listener.create_subscription<nav_msgs::msg::Path>("stereonet_plan", 10, [&](nav_msgs::msg::Path::ConstSharedPtr m) { path("plan", *m); });
  auto sub_arc =
      listener.create_subscription<nav_msgs::msg::Path>("stereonet_local_plan", 10, [&](nav_msgs::msg::Path::ConstSharedPtr m) { path("local_plan", *m); });
  auto sub_scan = listener.create_subscription<sensor_msgs::msg::LaserScan>("stereonet_scan", 10, [&](sensor_msgs::msg::LaserScan::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    std::ofstream o(file_of("scan"), std::ios::binary);
    o.write(reinterpret_cast<const char*>(m->ranges.data()), m->ranges.size() * sizeof(float));
    printf("scan seq=%d %s angle_min=%.9g angle_max=%.9g angle_increment=%.9g time_increment=%.9g scan_time=%.9g range_min=%.9g range_max=%.9g "
           "ranges=%zu intensities=%zu\n", seq, header(m->header).c_str(), m->angle_min, m->angle_max, m->angle_increment, m->time_increment,
           m->scan_time, m->range_min, m->range_max, m->ranges.size(), m->intensities.size());
    ++seq;
  });
  auto sub_cmd = listener.create_subscription<geometry_msgs::msg::Twist>("stereonet_cmd_vel", 10, [&](geometry_msgs::msg::Twist::ConstSharedPtr m) {
    std::lock_guard<std::mutex> lk(mu);
    printf("cmd seq=%d lx=%.17g ly=%.17g lz=%.17g ax=%.17g ay=%.17g az=%.17g\n", seq, m->linear.x, m->linear.y, m->linear.z, m->angular.x,
           m->angular.y, m->angular.z);
    ++seq;
  });
  auto sub_cloud =
      listener.create_subscription<sensor_msgs::msg::PointCloud2>("stereonet_pointcloud2", 10, [&](sensor_msgs::msg::PointCloud2::ConstSharedPtr m) {
        std::lock_guard<std::mutex> lk(mu);
        std::ofstream o(file_of("cloud"), std::ios::binary);
        o.write(reinterpret_cast<const char*>(m->data.data()), m->data.size());
        std::string fields;
        for (const auto& f : m->fields)
          fields += (fields.empty() ? "" : ",") + f.name + ":" + std::to_string(f.offset) + ":" + std::to_string((int)f.datatype) + ":" +
                    std::to_string(f.count);
        printf("cloud seq=%d %s height=%u width=%u point_step=%u row_step=%u is_dense=%d is_bigendian=%d fields=%s len=%zu\n", seq,
               header(m->header).c_str(), m->height, m->width, m->point_step, m->row_step, m->is_dense ? 1 : 0, m->is_bigendian ? 1 : 0, fields.c_str(),
               m->data.size());
        ++seq;
      });
  for (int k = 0; k < nframes; ++k) {
    node->SetBasePose(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2]);
    node->SetGoal(goal_x, goal_y);
    if (with_velocity) node->SetVelocity(vel_v, vel_w);
    auto done = std::async(std::launch::async, [&] {
      const int rc = node->Inject(raws.data() + (size_t)k * w * h, w, h, k);
      node->WaitIdle();
      return rc;
    });
    if (done.wait_for(std::chrono::seconds(60)) != std::future_status::ready) {
      fprintf(stderr, "timeout: frame %d of %d did not leave the node\n", k, nframes);
      fflush(stdout);
      _exit(4);      // the frame's thread is still inside the node: no destructor may wait for it
    }
    if (done.get() != 0) {
      fprintf(stderr, "PostProcess failed on frame %d\n", k);
      return 5;
    }
    std::lock_guard<std::mutex> lk(mu);
    printf("frame k=%d messages=%d\n", k, seq);
  }
  node.reset();
  rclcpp::shutdown();
  return 0;
}
