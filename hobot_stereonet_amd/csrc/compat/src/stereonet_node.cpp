// stereonet_node.cpp — live path of the stereo node, implemented over the dnn_node compat layer.
// Behavioural reference (what must stay observable from outside): stereonet_infer/src/stereonet_node.cpp
//   :24-127  parameters, Init, subscription + publishers      -> StereonetNode(), DeclareAndReadParameters()
//   :129-147 SetNodePara (model file must exist, task_num 4)  -> SetNodePara()
//   :657-818 FeedImg (validate, split eyes, tensor, JPEG, async Run) -> OnStereoFrame()
//   :980-1089 PostProcess (payload = raw tensor || JPEG, fps log)    -> PostProcess()
//   :820-976 RunImglistFeedInfer (offline file-list feeder)          -> RunImglistFeedInfer()
// The reference's other disabled feeders and dump helpers (:149-655) are not reproduced.
#include "stereonet_node.h"

#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "image_io.h"
#include "jpeg_nv12.h"
#include "jpeg_pool.h"
#include "stage_files.h"

namespace hobot {
namespace stereonet {

namespace {
const rclcpp::Logger kLog = rclcpp::get_logger("stereonet_node");

// STEREONET_NODE_STATS=1: average microseconds per frame of the node's own stages, printed when the process ends
struct StageStats {
  const bool on = getenv("STEREONET_NODE_STATS") != nullptr && atoi(getenv("STEREONET_NODE_STATS")) == 1;
  std::atomic<long> us[6] = {};
  std::atomic<long> n[6] = {};
  void add(int k, std::chrono::steady_clock::time_point t0) {
    if (!on) return;
    us[k] += (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    ++n[k];
  }
  ~StageStats() {
    if (!on) return;
    static const char* name[6] = {"FeedImg total", "FeedImg: queue JPEG", "FeedImg: Run (submit)", "PostProcess: wait for the JPEG",
                                  "PostProcess: build the message", "PostProcess: publish"};
    for (int k = 0; k < 6; ++k)
      if (n[k]) fprintf(stderr, "[node stats] %-34s %8.1f us/frame over %ld frames\n", name[k], (double)us[k] / n[k], (long)n[k]);
  }
};
StageStats g_stats;

int elapsed_ms(std::chrono::steady_clock::time_point since) {
  return (int)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - since).count();
}
}  // namespace

StereonetNode::StereonetNode(const std::string& node_name, const rclcpp::NodeOptions& options)
    : hobot::dnn_node::DnnNode(node_name, options) {
  DeclareAndReadParameters();

  // Init() calls SetNodePara() and loads the model; any failure ends the process the way the reference does
  if (Init() != 0 || GetModelInputSize(0, net_w_, net_h_) < 0) {
    RCLCPP_ERROR(kLog, "Node init fail!");
    rclcpp::shutdown();
    return;
  }
  net_ = GetModel();
  if (net_ == nullptr) {
    RCLCPP_ERROR(kLog, "Invalid model");
    rclcpp::shutdown();
    return;
  }
  LogModelIo();

  pre_.reset(new PreProcess(""));
  if (cfg_.publish_output) {
    int n = cfg_.jpeg_threads;
    if (const char* e = getenv("STEREONET_JPEG_THREADS")) n = atoi(e);
    if (n <= 0) {
      n = (int)std::thread::hardware_concurrency() / 4;
      n = n < 2 ? 2 : (n > 32 ? 32 : n);
    }
    jpeg_pool_ = std::make_shared<JpegPool>(n);
    if (const char* e = getenv("STEREONET_JPEG_SLICES")) cfg_.jpeg_slices = atoi(e);
    if (const char* e = getenv("STEREONET_JPEG")) cfg_.jpeg_gpu = !strcmp(e, "gpu");
    RCLCPP_WARN_STREAM(kLog, "left-eye JPEG encoder threads: " << n << ", slices per frame: " << cfg_.jpeg_slices
                                 << ", encoder: " << (cfg_.jpeg_gpu ? "gpu" : "host"));
  }
  frames_in_ = create_subscription<hbm_img_msgs::msg::HbmMsg1080P>(
      cfg_.image_topic, 10, [this](hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr m) { OnStereoFrame(m); });
  targets_out_ = create_publisher<ai_msgs::msg::PerceptionTargets>("/Stereonet_node_sample", 10);
  disparity_out_ = create_publisher<sensor_msgs::msg::Image>(cfg_.output_topic, 10);
  ReadRectifySettings();      // before the point cloud: its camera defaults to the rectifier's
  ReadPointCloudSettings();
  ReadRenderSettings();
  if (cfg_.render) render_out_ = create_publisher<sensor_msgs::msg::Image>("/image_jpeg", 10);
  if (cfg_.pointcloud_layout >= 0) pointcloud_out_ = create_publisher<sensor_msgs::msg::PointCloud2>("/stereonet_pointcloud2", 10);
  ReadObstacleSettings();
  ReadGroundSettings();
  if (cfg_.obstacles && cfg_.obstacle_params.gw)
    obstacle_grid_out_ = create_publisher<nav_msgs::msg::OccupancyGrid>("/stereonet_obstacle_grid", 10);
  if (cfg_.obstacles && cfg_.obstacle_params.beams)
    obstacle_scan_out_ = create_publisher<sensor_msgs::msg::LaserScan>("/stereonet_scan", 10);
  ReadCostmapSettings();
  ReadElevationSettings();
  ReadInflateSettings();
  ReadPlanSettings();
  ReadRolloutSettings();
  ReadTemporalSettings();
  ready_ = true;
}

StereonetNode::~StereonetNode() {
  if (!temporal_ && !rectify_ && !costmap_ && !elevation_) return;
  WaitIdle();      // requests in flight still pass through PostProcess; the engine is destroyed after the filter (~DnnNode)
  if (costmap_) sn_costmap_destroy(costmap_);
  costmap_ = nullptr;
  if (elevation_) sn_elevation_destroy(elevation_);
  elevation_ = nullptr;
  if (temporal_) sn_temporal_destroy(temporal_);
  temporal_ = nullptr;
  if (rectify_) sn_rectify_destroy(rectify_);
  rectify_ = nullptr;
}

void StereonetNode::DeclareAndReadParameters() {
  struct Item {
    const char* name;
    std::string* value;
  };
  const Item items[] = {{"config_file", &cfg_.config_file},
                        {"model_file", &cfg_.model_file},
                        {"sub_hbmem_topic_name", &cfg_.image_topic},
                        {"ros_img_topic_name", &cfg_.output_topic}};
  for (const Item& it : items) {
    declare_parameter<std::string>(it.name, *it.value);
    get_parameter<std::string>(it.name, *it.value);
  }
  if (const char* e = getenv("STEREONET_PUB_OUTPUT")) cfg_.publish_output = atoi(e) != 0;
  RCLCPP_WARN_STREAM(kLog, "\n config_file: " << cfg_.config_file << "\n model_file: " << cfg_.model_file
                                              << "\n sub_hbmem_topic_name: " << cfg_.image_topic
                                              << "\n ros_img_topic_name: " << cfg_.output_topic);
}

// cfg_.camera of the point cloud and the obstacle stage: the reference's intrinsics or the rectifier's, then STEREONET_CAMERA,
// STEREONET_POINTCLOUD_STEP and STEREONET_POINTCLOUD_Z.  false: *bad says which setting sn_pointcloud_from_raw would reject
bool StereonetNode::ReadCamera(std::string* bad_out) {
  std::string& bad = *bad_out;
  sn_camera& c = cfg_.camera;
  c = sn_camera{527.1931762695312f, 527.1931762695312f, net_w_ / 2.0f, net_h_ / 2.0f, 119.89382172f, 0.f, 0.f, 1};
  if (rectify_) sn_rectify_get_camera(rectify_, &c);      // the rectified left eye's; STEREONET_CAMERA still overrides it
  // checked once here: settings sn_pointcloud_from_raw would reject turn the stage off instead of failing every frame
  char end = 0;
  if (const char* v = getenv("STEREONET_CAMERA"))
    if (sscanf(v, "%f,%f,%f,%f,%f%c", &c.fx, &c.fy, &c.cx, &c.cy, &c.baseline_mm, &end) != 5)
      bad = std::string("STEREONET_CAMERA=") + v + " is not fx,fy,cx,cy,baseline_mm";
  if (const char* v = getenv("STEREONET_POINTCLOUD_STEP"))
    if (sscanf(v, "%d%c", &c.step, &end) != 1) bad = std::string("STEREONET_POINTCLOUD_STEP=") + v + " is not 1, 2 or 4";
  if (const char* v = getenv("STEREONET_POINTCLOUD_Z"))
    if (sscanf(v, "%f,%f%c", &c.z_min_m, &c.z_max_m, &end) != 2)
      bad = std::string("STEREONET_POINTCLOUD_Z=") + v + " is not min,max";
  if (bad.empty() && !(c.fx > 0.f && std::isfinite(c.fx) && c.fy > 0.f && std::isfinite(c.fy) && c.baseline_mm > 0.f &&
                       std::isfinite(c.cx) && std::isfinite(c.cy)))
    bad = "STEREONET_CAMERA: fx, fy and baseline_mm must be positive and every value finite";
  if (bad.empty() && c.step != 1 && c.step != 2 && c.step != 4) bad = "STEREONET_POINTCLOUD_STEP must be 1, 2 or 4";
  return bad.empty();
}

void StereonetNode::ReadPointCloudSettings() {
  const char* e = getenv("STEREONET_POINTCLOUD");
  if (!e || !*e) return;
  if (!strcmp(e, "organised")) {
    cfg_.pointcloud_layout = SN_PC_ORGANISED;
  } else if (!strcmp(e, "compact")) {
    cfg_.pointcloud_layout = SN_PC_COMPACT;
  } else {
    RCLCPP_ERROR_STREAM(kLog, "STEREONET_POINTCLOUD=" << e << " is neither organised nor compact: no point cloud");
    return;
  }
  std::string bad;
  ReadCamera(&bad);
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no point cloud");
    cfg_.pointcloud_layout = -1;
    return;
  }
  const sn_camera& c = cfg_.camera;
  RCLCPP_WARN_STREAM(kLog, "point cloud: " << e << " on /stereonet_pointcloud2, fx " << c.fx << " fy " << c.fy << " cx " << c.cx
                                           << " cy " << c.cy << " baseline_mm " << c.baseline_mm << " step " << c.step
                                           << " z " << c.z_min_m << ".." << c.z_max_m);
}

// read and validated once here: a file sn_rectify_create would reject leaves the node as it is without the variable
void StereonetNode::ReadRectifySettings() {
  const char* e = getenv("STEREONET_RECTIFY");
  if (!e || !*e) return;
  std::string bad;
  if (load_calib_file(e, &cfg_.calib, &bad) && sn_rectify_create(net_->engine(), &cfg_.calib, &rectify_) != SN_OK)
    bad = std::string("was refused: ") + sn_last_error(net_->engine());
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, "STEREONET_RECTIFY=" << e << " " << bad << ": no rectification");
    rectify_ = nullptr;
    return;
  }
  sn_rectify_info info{};
  sn_rectify_get_info(rectify_, &info);
  RCLCPP_WARN_STREAM(kLog, "rectification: raw frames of " << 2 * info.src_w << "x" << info.src_h << " -> " << 2 * info.w << "x"
                                                           << info.h << ", pixels with a source: left " << info.valid_left
                                                           << ", right " << info.valid_right);
}

// The raw side-by-side frame (2 src_w x src_h) -> a message of the model's size that holds the rectified frame and the raw
// one's index, stamp and encoding; everything downstream (ingest, the left-eye JPEG, the guide, the cloud's colour) then sees
// the rectified frame, with which the depth is aligned.  nullptr: not a frame of the calibration's size, or the call failed.
hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr StereonetNode::RectifyFrame(
    const hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr& raw) {
  const int sw = cfg_.calib.src_w, sh = cfg_.calib.src_h;
  if ((int)raw->height != sh || (int)raw->width != 2 * sw || raw->data.size() < (size_t)2 * sw * (sh + sh / 2)) {
    RCLCPP_ERROR_STREAM(kLog, "recved img msg h: " << raw->height << ", w: " << raw->width
                                                   << " is unmatch with the calibration's raw size " << 2 * sw << "x" << sh);
    return nullptr;
  }
  auto out = std::make_shared<hbm_img_msgs::msg::HbmMsg1080P>();
  out->index = raw->index;
  out->time_stamp = raw->time_stamp;
  out->encoding = raw->encoding;
  out->height = net_h_;
  out->width = 2 * net_w_;
  out->data.resize((size_t)3 * net_w_ * net_h_);
  out->data_size = (uint32_t)out->data.size();
  if (sn_rectify_nv12(rectify_, 1, raw->data.data(), raw->data.data() + sw, 2 * sw, 0, out->data.data(), nullptr, SN_MEM_HOST,
                      nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "rectification failed: %s", sn_last_error(net_->engine()));
    return nullptr;
  }
  return out;
}

// parsed and validated once here: a value sn_temporal_create would reject turns the filter off instead of failing every frame
void StereonetNode::ReadTemporalSettings() {
  const char* e = getenv("STEREONET_TEMPORAL");
  if (!e || !*e) return;
  sn_temporal_params& p = cfg_.temporal;
  p = sn_temporal_params{0, 0.f, 2, 0};
  int n2 = 0, n3 = 0, n4 = 0;      // characters used after 2, 3 and 4 fields: the whole value must be used
  const int got = sscanf(e, "%d,%f%n,%d%n,%d%n", &p.alpha, &p.delta_px, &n2, &p.persist, &n3, &p.luma_delta, &n4);
  const int used = got == 2 ? n2 : got == 3 ? n3 : got == 4 ? n4 : -1;
  std::string bad;
  if (used != (int)strlen(e))
    bad = "is not ALPHA,DELTA_PX[,PERSIST[,LUMA_DELTA]]";
  else if (p.alpha < 1 || p.alpha > 256 || !std::isfinite(p.delta_px) || p.delta_px < 0.f || p.persist < 0 || p.persist > 8 ||
           p.luma_delta < 0 || p.luma_delta > 255)
    bad = "needs ALPHA 1..256, DELTA_PX finite and >= 0, PERSIST 0..8, LUMA_DELTA 0..255";
  else if (sn_temporal_create(net_->engine(), 1, &p, &temporal_) != SN_OK)
    bad = std::string("was refused: ") + sn_last_error(net_->engine());
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, "STEREONET_TEMPORAL=" << e << " " << bad << ": no temporal filter");
    temporal_ = nullptr;
    return;
  }
  RCLCPP_WARN_STREAM(kLog, "temporal filter: alpha " << p.alpha << "/256, delta_px " << p.delta_px << ", persist " << p.persist
                                                     << ", luma_delta " << p.luma_delta);
}

// whether the request carries a side-by-side NV12 frame of the model's size (the offline feeder's requests carry none)
bool StereonetNode::HasModelFrame(const StereonetNodeOutput& request) const {
  const auto& f = request.frame;
  return f && (int)f->width == 2 * net_w_ && (int)f->height == net_h_ &&
         f->data.size() >= (size_t)2 * net_w_ * (net_h_ + (net_h_ + 1) / 2);
}

// The request's int32 tensor, filtered in place as the next frame of the node's one stream.  DnnNode::CompletionLoop calls
// PostProcess from one thread in submission order, and the synchronous path calls it inline, so the pushes arrive in frame
// order.  With LUMA_DELTA > 0 the guide is the request's side-by-side frame (NV12, pitch 2W).  A request without a frame of
// the model's size (the offline feeder's) has no luma to compare: its map passes UNFILTERED and the stream is reset, so the
// next guided frame starts afresh instead of being blended across the gap.
void StereonetNode::FilterTemporal(const StereonetNodeOutput& request, int32_t* raw) {
  const auto& f = request.frame;
  const uint8_t* guide = nullptr;
  if (cfg_.temporal.luma_delta > 0) {
    if (!HasModelFrame(request)) {
      if (!temporal_unguided_logged_)
        RCLCPP_WARN(kLog, "temporal filter: no side-by-side frame of the model's size for this request, map not filtered");
      temporal_unguided_logged_ = true;
      sn_temporal_reset(temporal_, 0);
      return;
    }
    guide = f->data.data();
  }
  if (sn_temporal_push(temporal_, 1, nullptr, raw, guide, SN_GUIDE_NV12, 2 * net_w_, raw, nullptr, nullptr, nullptr, SN_MEM_HOST,
                       nullptr) != SN_OK)
    RCLCPP_ERROR(kLog, "temporal filter failed: %s", sn_last_error(net_->engine()));
}

// parsed and validated once here: a value sn_render_jpeg would refuse leaves the node as it is without the variable
void StereonetNode::ReadRenderSettings() {
  const char* e = getenv("STEREONET_RENDER");
  if (!e || !*e) return;
  sn_jpeg_params& jp = cfg_.render_jpeg;
  jp = sn_jpeg_params{95, 1};
  int n1 = 0, n2 = 0;      // characters used after 1 and 2 fields: the whole value must be used
  const int got = sscanf(e, "%d%n,%d%n", &jp.quality, &n1, &jp.rows_per_slice, &n2);
  const int used = got == 1 ? n1 : got == 2 ? n2 : -1;
  std::string bad;
  if (used != (int)strlen(e)) bad = "is not Q[,ROWS]";
  else if (jp.quality < 1 || jp.quality > 100 || jp.rows_per_slice < 0) bad = "needs Q 1..100 and ROWS >= 0";
  else if (((net_w_ | net_h_) & 1) || sn_jpeg_bound(net_w_, 2 * net_h_) == 0) bad = "needs a model of even width and height";
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, "STEREONET_RENDER=" << e << " " << bad << ": no depth view");
    return;
  }
  auto flag = [](const char* name) { return getenv(name) != nullptr && atoi(getenv(name)) == 1; };
  cfg_.render_params = sn_render_params{};      // the reference's render node
  cfg_.render_params.true_colours = flag("STEREONET_RENDER_TRUE");
  cfg_.render_params.invalid_black = flag("STEREONET_RENDER_INVALID_BLACK");
  cfg_.render = true;
  RCLCPP_WARN_STREAM(kLog, "depth view on /image_jpeg: quality " << jp.quality << ", rows per slice " << jp.rows_per_slice
                                                                 << ", true colours " << cfg_.render_params.true_colours
                                                                 << ", invalid black " << cfg_.render_params.invalid_black);
}

// sensor_msgs/Image on /image_jpeg as the reference render node's cv2_to_imgmsg forms it: encoding "jpeg", width W, height 2H,
// step = the data's length; data = the JPEG of the request's left eye (the rectified one where the node rectifies) over its
// colour-mapped map, by one sn_render_jpeg call.  A request without a side-by-side frame of the model's size (the offline
// feeder's) has no left eye in NV12: nothing is published for it.
void StereonetNode::PublishRender(const StereonetNodeOutput& request, const int32_t* raw) {
  const auto& f = request.frame;
  if (!HasModelFrame(request)) {
    if (!render_no_frame_logged_.exchange(true))
      RCLCPP_WARN(kLog, "depth view: no side-by-side frame of the model's size for this request, nothing published");
    return;
  }
  sensor_msgs::msg::Image msg;
  msg.header = *request.msg_header;
  msg.width = net_w_;
  msg.height = 2 * net_h_;
  msg.encoding = "jpeg";
  msg.data.resize(sn_jpeg_bound(net_w_, 2 * net_h_));
  uint32_t size = 0;
  const int rc = sn_render_jpeg(net_->engine(), 1, raw, f->data.data(), 2 * net_w_, &cfg_.render_params, &cfg_.render_jpeg,
                                msg.data.data(), msg.data.size(), &size, SN_MEM_HOST, nullptr);
  if (rc != SN_OK || size == 0) {
    RCLCPP_ERROR(kLog, "depth view failed: %s", rc != SN_OK ? sn_last_error(net_->engine()) : "the stream did not fit");
    return;
  }
  msg.data.resize(size);
  msg.step = size;
  render_out_->publish(std::move(msg));
}

// sensor_msgs/PointCloud2 of the request's map: x, y, z (+ rgb) FLOAT32 at 0 / 4 / 8 / 12, 16 bytes a point, the header of
// the disparity message; organised = the sampled image grid with NaN for invalid samples, compact = one row of valid points
void StereonetNode::PublishPointCloud(const StereonetNodeOutput& request, const int32_t* raw) {
  const sn_camera& cam = cfg_.camera;
  const int wo = (net_w_ + cam.step - 1) / cam.step, ho = (net_h_ + cam.step - 1) / cam.step;
  const auto& f = request.frame;
  const bool colour = HasModelFrame(request);
  if (!colour && !cloud_uncoloured_logged_.exchange(true))
    RCLCPP_WARN(kLog, "point cloud without colour: no side-by-side frame of the model's size for this request");
  sensor_msgs::msg::PointCloud2 msg;
  msg.header = *request.msg_header;
  msg.data.resize((size_t)ho * wo * 16);
  uint32_t count = 0;
  const int rc = sn_pointcloud_from_raw(net_->engine(), 1, raw, colour ? f->data.data() : nullptr, 2 * net_w_, &cam,
                                        cfg_.pointcloud_layout, reinterpret_cast<float*>(msg.data.data()), &count,
                                        SN_MEM_HOST, nullptr);
  if (rc != SN_OK) {
    RCLCPP_ERROR(kLog, "point cloud failed: %s", sn_last_error(net_->engine()));
    return;
  }
  const char* names[4] = {"x", "y", "z", "rgb"};
  for (int k = 0; k < (colour ? 4 : 3); ++k) {
    sensor_msgs::msg::PointField pf;
    pf.name = names[k];
    pf.offset = 4 * k;
    pf.datatype = sensor_msgs::msg::PointField::FLOAT32;
    pf.count = 1;
    msg.fields.push_back(pf);
  }
  msg.is_bigendian = false;
  msg.point_step = 16;
  if (cfg_.pointcloud_layout == SN_PC_ORGANISED) {
    msg.height = ho;
    msg.width = wo;
    msg.is_dense = false;
  } else {
    msg.height = 1;
    msg.width = count;
    msg.is_dense = true;
    msg.data.resize((size_t)count * 16);
  }
  msg.row_step = 16 * msg.width;
  pointcloud_out_->publish(std::move(msg));
}

void StereonetNode::ReadObstacleSettings() {
  const char* e = getenv("STEREONET_OBSTACLES");
  if (!e || !*e) return;
  sn_obstacle_params& p = cfg_.obstacle_params;
  p = default_obstacle_params();
  std::string bad;
  if (!load_obstacle_file(e, &p, &cfg_.obstacle_frame, &bad)) bad = std::string("STEREONET_OBSTACLES=") + e + ": " + bad;
  if (bad.empty() && cfg_.pointcloud_layout < 0) ReadCamera(&bad);      // the point cloud's camera, read once
  // checked once here, on empty buffers: what sn_obstacles_from_raw would refuse turns the stage off instead of failing every frame
  std::vector<float> edges(p.beams > 0 && p.beams <= 4096 ? p.beams + 1 : 0);
  if (bad.empty() && !p.gw && !p.beams) bad = "neither a grid (gw, gh) nor a scan (beams)";
  if (bad.empty() && p.beams && (edges.empty() || sn_obstacle_beam_edges(&p, edges.data()) != SN_OK))
    bad = "the sector must have 1..4096 beams inside (-pi/2, pi/2)";
  if (bad.empty()) {
    std::vector<int32_t> none((size_t)net_w_ * net_h_, 0);
    std::vector<uint32_t> hits((size_t)p.gw * p.gh * 2);
    std::vector<float> ranges(p.beams);
    if (sn_obstacles_from_raw(net_->engine(), 1, none.data(), &cfg_.camera, &p, nullptr, p.gw ? hits.data() : nullptr, nullptr,
                              p.beams ? ranges.data() : nullptr, nullptr, SN_MEM_HOST, nullptr) != SN_OK)
      bad = sn_last_error(net_->engine());
  }
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no obstacle grid and no scan");
    return;
  }
  cfg_.obstacles = true;
  RCLCPP_WARN_STREAM(kLog, "obstacles: frame " << cfg_.obstacle_frame << ", grid " << p.gw << " x " << p.gh << " cells of " << p.cell_m
                                               << " m on /stereonet_obstacle_grid, " << p.beams << " beams on /stereonet_scan");
}

// nav_msgs/OccupancyGrid and sensor_msgs/LaserScan of the request's map: one sn_obstacles_from_raw call, the stamp of the
// disparity message, the frame of the parameter file
void StereonetNode::PublishObstacles(const StereonetNodeOutput& request, const int32_t* raw, const float* mount) {
  const sn_obstacle_params& p = cfg_.obstacle_params;
  nav_msgs::msg::OccupancyGrid grid;
  sensor_msgs::msg::LaserScan scan;
  grid.data.resize((size_t)p.gw * p.gh);
  scan.ranges.resize(p.beams);
  int8_t* occ = p.gw ? grid.data.data() : nullptr;
  float* ranges = p.beams ? scan.ranges.data() : nullptr;
  const int rc = mount ? sn_obstacles_from_raw_mounts(net_->engine(), 1, raw, &cfg_.camera, &p, mount, 12, occ, nullptr, nullptr, ranges,
                                                      nullptr, SN_MEM_HOST, nullptr)      // the frame's mount, from FitGround
                       : sn_obstacles_from_raw(net_->engine(), 1, raw, &cfg_.camera, &p, occ, nullptr, nullptr, ranges, nullptr,
                                               SN_MEM_HOST, nullptr);
  if (rc != SN_OK) {
    RCLCPP_ERROR(kLog, "obstacles failed: %s", sn_last_error(net_->engine()));
    return;
  }
  // the costmap and the inflation read the frame's grid and scan after the messages that own them have left
  nav_msgs::msg::OccupancyGrid inflate_src;
  std::vector<int8_t> occ_kept;
  std::vector<float> ranges_kept;
  if (costmap_) {
    occ_kept = grid.data;
    ranges_kept = scan.ranges;
  }
  if (obstacle_grid_out_) {
    grid.header.stamp = request.msg_header->stamp;
    grid.header.frame_id = cfg_.obstacle_frame;
    grid.info.map_load_time = request.msg_header->stamp;
    grid.info.resolution = p.cell_m;
    grid.info.width = p.gw;
    grid.info.height = p.gh;
    grid.info.origin.position.x = p.x_min_m;
    grid.info.origin.position.y = p.y_min_m;
    const bool feeds = cfg_.inflate && !costmap_ && !cfg_.elevation_feeds_inflate;
    if (feeds) inflate_src = grid;      // the inflated grid follows this one
    obstacle_grid_out_->publish(std::move(grid));
    if (feeds) PublishInflated(inflate_src);
  }
  if (obstacle_scan_out_) {
    scan.header.stamp = request.msg_header->stamp;
    scan.header.frame_id = cfg_.obstacle_frame;
    scan.angle_min = p.angle_min_rad + 0.5f * p.angle_increment_rad;      // beam i looks along the middle of its sector
    scan.angle_increment = p.angle_increment_rad;
    scan.angle_max = scan.angle_min + (float)(p.beams - 1) * p.angle_increment_rad;
    scan.range_min = p.range_min_m;
    scan.range_max = p.range_max_m;
    obstacle_scan_out_->publish(std::move(scan));
  }
  if (costmap_) PublishCostmap(request, p.gw ? occ_kept.data() : nullptr, p.beams ? ranges_kept.data() : nullptr);
}

// parsed and validated once here: what sn_costmap_create would refuse turns the stage off instead of failing every frame
void StereonetNode::ReadCostmapSettings() {
  const char* e = getenv("STEREONET_COSTMAP");
  if (!e || !*e) return;
  sn_costmap_params& p = cfg_.costmap_params;
  p = default_costmap_params();
  std::string bad;
  if (!cfg_.obstacles) bad = std::string("STEREONET_COSTMAP=") + e + " requires STEREONET_OBSTACLES";
  else if (!load_costmap_file(e, &p, &cfg_.costmap_frame, &bad)) bad = std::string("STEREONET_COSTMAP=") + e + ": " + bad;
  else if (sn_costmap_create(net_->engine(), 1, &cfg_.obstacle_params, &p, &costmap_) != SN_OK) bad = sn_last_error(net_->engine());
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no costmap");
    costmap_ = nullptr;
    return;
  }
  costmap_out_ = create_publisher<nav_msgs::msg::OccupancyGrid>("/stereonet_costmap", 10);
  RCLCPP_WARN_STREAM(kLog, "costmap: frame " << cfg_.costmap_frame << ", window " << p.mw << " x " << p.mh << " cells of "
                                             << cfg_.obstacle_params.cell_m << " m on /stereonet_costmap, hit " << p.l_hit << ", miss "
                                             << p.l_miss << ", clamps " << p.l_min << " .. " << p.l_max);
}

void StereonetNode::SetBasePose(double x, double y, double yaw) {
  std::lock_guard<std::mutex> lk(base_pose_mu_);
  base_pose_[0] = x, base_pose_[1] = y, base_pose_[2] = yaw;
}

// nav_msgs/OccupancyGrid of the rolling map after this frame: one sn_costmap_push call at the pose of SetBasePose, the stamp of
// the disparity message, the origin of the window from the quantised pose
void StereonetNode::PublishCostmap(const StereonetNodeOutput& request, const int8_t* occ, const float* ranges) {
  const sn_costmap_params& p = cfg_.costmap_params;
  double pose[3];
  {
    std::lock_guard<std::mutex> lk(base_pose_mu_);
    memcpy(pose, base_pose_, sizeof(pose));
  }
  nav_msgs::msg::OccupancyGrid map;
  map.data.resize((size_t)p.mw * p.mh);
  int32_t q[6];
  if (sn_costmap_push(costmap_, 1, nullptr, pose, occ, ranges, map.data.data(), nullptr, nullptr, q, SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "costmap failed: %s", sn_last_error(net_->engine()));
    return;
  }
  map.header.stamp = request.msg_header->stamp;
  map.header.frame_id = cfg_.costmap_frame;
  map.info.map_load_time = request.msg_header->stamp;
  map.info.resolution = cfg_.obstacle_params.cell_m;
  map.info.width = p.mw;
  map.info.height = p.mh;
  map.info.origin.position.x = (double)q[4] * (double)cfg_.obstacle_params.cell_m;
  map.info.origin.position.y = (double)q[5] * (double)cfg_.obstacle_params.cell_m;
  nav_msgs::msg::OccupancyGrid inflate_src;
  const bool feeds = cfg_.inflate && !cfg_.elevation_feeds_inflate;
  if (feeds) inflate_src = map;      // the inflated grid follows this one
  costmap_out_->publish(std::move(map));
  if (feeds) PublishInflated(inflate_src);
}

// parsed and validated once here: what sn_elevation_create would refuse turns the stage off instead of failing every frame
void StereonetNode::ReadElevationSettings() {
  const char* e = getenv("STEREONET_ELEVATION");
  if (!e || !*e) return;
  sn_elevation_params& p = cfg_.elevation_params;
  p = default_elevation_params();
  std::string bad;
  bool feed = false;
  if (!load_elevation_file(e, &p, &cfg_.elevation_frame, &feed, &bad)) bad = std::string("STEREONET_ELEVATION=") + e + ": " + bad;
  if (bad.empty() && cfg_.pointcloud_layout < 0 && !cfg_.obstacles && !cfg_.ground) ReadCamera(&bad);      // the point cloud's camera, read once
  if (bad.empty() && sn_elevation_create(net_->engine(), 1, &p, &elevation_) != SN_OK) bad = sn_last_error(net_->engine());
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no elevation map");
    elevation_ = nullptr;
    return;
  }
  cfg_.elevation_feeds_inflate = feed;
  traversability_out_ = create_publisher<nav_msgs::msg::OccupancyGrid>("/stereonet_traversability", 10);
  RCLCPP_WARN_STREAM(kLog, "elevation: frame " << cfg_.elevation_frame << ", window " << p.mw << " x " << p.mh << " cells of " << p.cell_m
                                               << " m on /stereonet_traversability, step " << p.max_step_mm << " mm over radius " << p.radius
                                               << ", alpha " << p.alpha << (feed ? ", feeding the inflation" : ""));
}

// nav_msgs/OccupancyGrid of the traversability verdict after this frame: one sn_elevation_push call at the pose of SetBasePose
// (with the frame's mount, from FitGround, where there is one), the stamp of the disparity message, the origin of the window
// from the quantised pose
void StereonetNode::PublishElevation(const StereonetNodeOutput& request, const int32_t* raw, const float* mount) {
  const sn_elevation_params& p = cfg_.elevation_params;
  double pose[3];
  {
    std::lock_guard<std::mutex> lk(base_pose_mu_);
    memcpy(pose, base_pose_, sizeof(pose));
  }
  nav_msgs::msg::OccupancyGrid map;
  map.data.resize((size_t)p.mw * p.mh);
  int32_t q[6];
  if (sn_elevation_push(elevation_, 1, nullptr, pose, raw, &cfg_.camera, mount, 12, map.data.data(), nullptr, nullptr, nullptr, nullptr, q,
                        SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "elevation failed: %s", sn_last_error(net_->engine()));
    return;
  }
  map.header.stamp = request.msg_header->stamp;
  map.header.frame_id = cfg_.elevation_frame;
  map.info.map_load_time = request.msg_header->stamp;
  map.info.resolution = p.cell_m;
  map.info.width = p.mw;
  map.info.height = p.mh;
  map.info.origin.position.x = (double)q[4] * (double)p.cell_m;
  map.info.origin.position.y = (double)q[5] * (double)p.cell_m;
  nav_msgs::msg::OccupancyGrid inflate_src;
  const bool feeds = cfg_.inflate && cfg_.elevation_feeds_inflate;
  if (feeds) inflate_src = map;      // the inflated grid follows this one
  traversability_out_->publish(std::move(map));
  if (feeds) PublishInflated(inflate_src);
}

// parsed and validated once here: what sn_inflate_grid would refuse turns the stage off instead of failing every frame
void StereonetNode::ReadInflateSettings() {
  const char* e = getenv("STEREONET_INFLATE");
  if (!e || !*e) return;
  // the cell is that of the grid the stage follows, whatever the file says
  sn_inflate_params& p = cfg_.inflate_params;
  p = default_inflate_params();
  std::string bad;
  int R = 0;
  const bool from_elevation = elevation_ && cfg_.elevation_feeds_inflate;
  if (!from_elevation && (!cfg_.obstacles || !cfg_.obstacle_params.gw))
    bad = std::string("STEREONET_INFLATE=") + e + " requires STEREONET_OBSTACLES with a grid";
  else if (!load_inflate_file(e, &p, &bad)) bad = std::string("STEREONET_INFLATE=") + e + ": " + bad;
  else {
    p.cell_m = from_elevation ? cfg_.elevation_params.cell_m : cfg_.obstacle_params.cell_m;
    if (sn_inflate_table(&p, nullptr, &R) != SN_OK) bad = std::string("STEREONET_INFLATE=") + e + ": parameters sn_inflate_table refuses";
  }
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no inflated grid");
    return;
  }
  cfg_.inflate = true;
  inflated_out_ = create_publisher<nav_msgs::msg::OccupancyGrid>("/stereonet_inflated_grid", 10);
  RCLCPP_WARN_STREAM(kLog, "inflation: " << (from_elevation ? "/stereonet_traversability" : costmap_ ? "/stereonet_costmap" : "/stereonet_obstacle_grid")
                                         << " on /stereonet_inflated_grid, inscribed "
                                         << p.inscribed_radius_m << " m, out to " << p.inflation_radius_m << " m (" << R << " cells), scaling "
                                         << p.cost_scaling << ", lethal from " << p.lethal_min);
}

// nav_msgs/OccupancyGrid of the costs after inflation: one sn_inflate_grid call on the grid just published, whose header and
// info it takes
void StereonetNode::PublishInflated(const nav_msgs::msg::OccupancyGrid& src) {
  nav_msgs::msg::OccupancyGrid out;
  out.header = src.header;
  out.info = src.info;
  out.data.resize(src.data.size());
  std::vector<uint8_t> cost(cfg_.plan ? src.data.size() : 0);      // the plan reads the cost bytes, not their translation
  if (sn_inflate_grid(net_->engine(), 1, src.data.data(), (int)src.info.width, (int)src.info.height, &cfg_.inflate_params,
                      cfg_.plan ? cost.data() : nullptr, out.data.data(), nullptr, nullptr, SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "inflation failed: %s", sn_last_error(net_->engine()));
    return;
  }
  inflated_out_->publish(std::move(out));
  if (cfg_.plan) PublishPlan(src, cost.data());
}

// parsed and validated once here: what sn_navfn would refuse turns the stage off instead of failing every frame
void StereonetNode::ReadPlanSettings() {
  const char* e = getenv("STEREONET_PLAN");
  if (!e || !*e) return;
  sn_nav_params& p = cfg_.plan_params;
  p = default_plan_params();
  std::string bad;
  if (!cfg_.inflate) bad = std::string("STEREONET_PLAN=") + e + " requires STEREONET_INFLATE";
  else if (!load_plan_file(e, &p, &bad)) bad = std::string("STEREONET_PLAN=") + e + ": " + bad;
  else if (p.neutral < 1 || p.neutral > 255 || p.lethal_cost < 1 || p.lethal_cost > 255 || p.unknown_cost < 0 || p.unknown_cost > 252 ||
           (p.flags & ~SN_NAV_UNKNOWN_OK) || p.max_rounds < 0 || p.max_path < 1 || p.max_path > SN_NAV_MAX_CELLS)
    bad = std::string("STEREONET_PLAN=") + e + ": parameters sn_navfn refuses, or max_path outside 1..2^20 (no path is longer than a grid has cells)";
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no plan");
    return;
  }
  cfg_.plan = true;
  plan_out_ = create_publisher<nav_msgs::msg::Path>("/stereonet_plan", 10);
  RCLCPP_WARN_STREAM(kLog, "plan: /stereonet_inflated_grid to the goal of SetGoal on /stereonet_plan, neutral " << p.neutral << ", lethal from "
                                                                                                                  << p.lethal_cost << ", at most " << p.max_path
                                                                                                                  << " cells");
}

void StereonetNode::SetGoal(double x_m, double y_m) {
  std::lock_guard<std::mutex> lk(base_pose_mu_);
  goal_[0] = x_m, goal_[1] = y_m;
  has_goal_ = true;
}

// nav_msgs/Path from the robot's cell to the goal's over the costs just made: one sn_navfn call; the header of the grid's source
void StereonetNode::PublishPlan(const nav_msgs::msg::OccupancyGrid& src, const uint8_t* cost) {
  double goal[2], robot[2] = {0.0, 0.0};      // the obstacle grid is in the base frame: the robot stands at its origin
  {
    std::lock_guard<std::mutex> lk(base_pose_mu_);
    if (!has_goal_) return;
    memcpy(goal, goal_, sizeof(goal));
    if (costmap_ || cfg_.elevation_feeds_inflate) robot[0] = base_pose_[0], robot[1] = base_pose_[1];      // a grid in the fixed frame
  }
  const int gw = (int)src.info.width, gh = (int)src.info.height;
  const double res = (double)src.info.resolution, ox = src.info.origin.position.x, oy = src.info.origin.position.y;
  auto cell_of = [&](const double at[2], int32_t out[2]) {      // -> whether a coordinate was clamped
    const double fx = std::floor((at[0] - ox) / res), fy = std::floor((at[1] - oy) / res);
    const double cx = std::min(std::max(fx, 0.0), (double)(gw - 1)), cy = std::min(std::max(fy, 0.0), (double)(gh - 1));
    out[0] = (int32_t)cx, out[1] = (int32_t)cy;
    return cx != fx || cy != fy;
  };
  int32_t g[2], s[2];
  if (cell_of(goal, g) && !goal_clamp_logged_.exchange(true))
    RCLCPP_WARN(kLog, "plan: the goal (%.3f, %.3f) lies outside the grid and is clamped to cell (%d, %d)", goal[0], goal[1], g[0], g[1]);
  cell_of(robot, s);
  // allocated once per thread that publishes, not per frame; max_path was bounded at start-up
  thread_local std::vector<int32_t> cells;
  cells.resize((size_t)cfg_.plan_params.max_path * 2);
  thread_local std::vector<uint32_t> potential;      // the rollout scores its arcs by it
  if (cfg_.rollout) potential.resize((size_t)gw * gh);
  uint32_t stats[5];
  if (sn_navfn(net_->engine(), 1, cost, gw, gh, g, s, &cfg_.plan_params, cfg_.rollout ? potential.data() : nullptr, cells.data(), stats, nullptr,
               SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "plan failed: %s", sn_last_error(net_->engine()));
    return;
  }
  nav_msgs::msg::Path out;
  out.header = src.header;
  const size_t n = std::min<size_t>(stats[2], (size_t)cfg_.plan_params.max_path);
  out.poses.resize(n);
  for (size_t i = 0; i < n; ++i) {
    out.poses[i].header = src.header;
    out.poses[i].pose.position.x = ox + ((double)cells[2 * i] + 0.5) * res;
    out.poses[i].pose.position.y = oy + ((double)cells[2 * i + 1] + 0.5) * res;
  }
  if (stats[0]) RCLCPP_DEBUG(kLog, "plan: flags %u, %u cells", stats[0], stats[2]);
  plan_out_->publish(std::move(out));
  if (cfg_.rollout) PublishRollout(src, cost, potential.data());
}

namespace {
// one axis of rollout.window_from_velocity: the lattice samples within `reach` of `at`, else the one nearest to it (the lower
// on a tie); lattice(i) is sn_rollout_velocity's
void window_axis(const sn_rollout_params& p, bool turn, double at, double reach, int32_t* lo, int32_t* hi) {
  const int count = turn ? p.nw : p.nv;
  int first = -1, last = -1, near = 0;
  double near_d = 0.0;
  for (int i = 0; i < count; ++i) {
    double vw[2];
    sn_rollout_velocity(&p, turn ? i : i * p.nw, vw);
    const double l = vw[turn ? 1 : 0], d = std::fabs(l - at);
    if (l >= at - reach && l <= at + reach) {
      if (first < 0) first = i;
      last = i;
    }
    if (i == 0 || d < near_d) near = i, near_d = d;
  }
  *lo = first < 0 ? near : first, *hi = first < 0 ? near : last;
}
}  // namespace

// parsed and validated once here: what sn_rollout would refuse turns the stage off instead of failing every frame
void StereonetNode::ReadRolloutSettings() {
  const char* e = getenv("STEREONET_ROLLOUT");
  if (!e || !*e) return;
  sn_rollout_params& p = cfg_.rollout_params;
  p = default_rollout_params();
  std::string bad;
  const double* a = cfg_.rollout_acc;
  if (!cfg_.plan) bad = std::string("STEREONET_ROLLOUT=") + e + " requires STEREONET_PLAN";
  else if (!load_rollout_file(e, &p, &cfg_.rollout_footprint, cfg_.rollout_acc, &cfg_.rollout_has_acc, &bad))
    bad = std::string("STEREONET_ROLLOUT=") + e + ": " + bad;
  else if (cfg_.rollout_footprint.size() > 2 * SN_ROLLOUT_MAX_POINTS ||
           sn_rollout_tables(&p, cfg_.rollout_footprint.data(), (int)cfg_.rollout_footprint.size() / 2, nullptr, nullptr) != SN_OK)
    bad = std::string("STEREONET_ROLLOUT=") + e + ": parameters or a footprint sn_rollout refuses";
  else if (cfg_.rollout_has_acc && !(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && a[0] >= 0.0 && a[1] >= 0.0 && a[2] >= 0.0))
    bad = std::string("STEREONET_ROLLOUT=") + e + ": acc_v, acc_w and dt must be finite and not negative";
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no velocity command");
    return;
  }
  cfg_.rollout = true;
  cmd_vel_out_ = create_publisher<geometry_msgs::msg::Twist>("/stereonet_cmd_vel", 10);
  local_plan_out_ = create_publisher<nav_msgs::msg::Path>("/stereonet_local_plan", 10);
  RCLCPP_WARN_STREAM(kLog, "rollout: " << p.nv << " x " << p.nw << " samples over " << p.sim_time_s << " s in " << p.steps << " steps, "
                                       << cfg_.rollout_footprint.size() / 2 << " footprint points, on /stereonet_cmd_vel and /stereonet_local_plan");
}

void StereonetNode::SetVelocity(double v, double w) {
  std::lock_guard<std::mutex> lk(base_pose_mu_);
  velocity_[0] = v, velocity_[1] = w;
  has_velocity_ = true;
}

// geometry_msgs/Twist and nav_msgs/Path of the best velocity sample over the costs and the potential just made: one sn_rollout
// call.  A frame whose pose or grid the call refuses, like one without a valid sample, commands a stop.
void StereonetNode::PublishRollout(const nav_msgs::msg::OccupancyGrid& src, const uint8_t* cost, const uint32_t* potential) {
  double pose[3] = {0.0, 0.0, 0.0}, vel[2];      // the obstacle grid is in the base frame: the robot stands at its origin, heading along x
  bool moving;
  {
    std::lock_guard<std::mutex> lk(base_pose_mu_);
    if (costmap_ || cfg_.elevation_feeds_inflate) memcpy(pose, base_pose_, sizeof(pose));      // a grid in the fixed frame
    memcpy(vel, velocity_, sizeof(vel));
    moving = has_velocity_;
  }
  const int gw = (int)src.info.width, gh = (int)src.info.height;
  const double ox = src.info.origin.position.x, oy = src.info.origin.position.y;
  sn_rollout_params p = cfg_.rollout_params;
  p.cell_m = src.info.resolution;
  const double cell = (double)p.cell_m;
  int32_t q[5], window[4];
  const bool windowed = moving && cfg_.rollout_has_acc && std::isfinite(vel[0]) && std::isfinite(vel[1]);
  if (windowed) {
    window_axis(p, false, vel[0], cfg_.rollout_acc[0] * cfg_.rollout_acc[2], &window[0], &window[1]);
    window_axis(p, true, vel[1], cfg_.rollout_acc[1] * cfg_.rollout_acc[2], &window[2], &window[3]);
  }
  thread_local std::vector<int32_t> traj;
  traj.resize((size_t)(p.steps + 1) * 3);
  uint32_t best[8] = {SN_ROLLOUT_NO_VALID};
  geometry_msgs::msg::Twist cmd;
  nav_msgs::msg::Path arc;
  arc.header = src.header;
  if (sn_rollout_pose_q(p.cell_m, ox, oy, pose, q) != SN_OK) {
    RCLCPP_ERROR(kLog, "rollout: the pose (%.3f, %.3f, %.3f) cannot be placed on the grid", pose[0], pose[1], pose[2]);
  } else if (sn_rollout(net_->engine(), 1, cost, potential, gw, gh, q, windowed ? window : nullptr, &p, cfg_.rollout_footprint.data(),
                        (int)cfg_.rollout_footprint.size() / 2, nullptr, best, traj.data(), SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "rollout failed: %s", sn_last_error(net_->engine()));
    best[0] = SN_ROLLOUT_NO_VALID;
  }
  if (!(best[0] & SN_ROLLOUT_NO_VALID)) {
    double vw[2];
    sn_rollout_velocity(&p, (int)best[1], vw);
    cmd.linear.x = vw[0], cmd.angular.z = vw[1];
    arc.poses.resize((size_t)p.steps + 1);
    for (size_t t = 0; t < arc.poses.size(); ++t) {
      const double half = (double)traj[3 * t + 2] / 65536.0 * 3.141592653589793;      // half the heading, in radians
      arc.poses[t].header = src.header;
      arc.poses[t].pose.position.x = ox + (double)traj[3 * t] / 256.0 * cell;
      arc.poses[t].pose.position.y = oy + (double)traj[3 * t + 1] / 256.0 * cell;
      arc.poses[t].pose.orientation.z = std::sin(half), arc.poses[t].pose.orientation.w = std::cos(half);
    }
  } else {
    RCLCPP_DEBUG(kLog, "rollout: no valid sample (%u collide, %u without a route, %u outside the window)", best[5], best[6], best[7]);
  }
  cmd_vel_out_->publish(std::move(cmd));
  local_plan_out_->publish(std::move(arc));
}

void StereonetNode::ReadGroundSettings() {
  const char* e = getenv("STEREONET_GROUND");
  if (!e || !*e) return;
  sn_ground_params& p = cfg_.ground_params;
  p = default_ground_params();
  std::string bad;
  if (!load_ground_file(e, &p, &cfg_.ground_log_delta, &bad)) bad = std::string("STEREONET_GROUND=") + e + ": " + bad;
  if (bad.empty() && cfg_.pointcloud_layout < 0 && !cfg_.obstacles) ReadCamera(&bad);      // the point cloud's camera, read once
  // checked once here, on an empty map: what sn_ground_from_raw would refuse turns the stage off instead of failing every frame
  if (bad.empty()) {
    std::vector<int32_t> none((size_t)net_w_ * net_h_, 0);
    sn_ground g;
    if (sn_ground_from_raw(net_->engine(), 1, none.data(), &cfg_.camera, &p, &g, nullptr, SN_MEM_HOST, nullptr) != SN_OK)
      bad = sn_last_error(net_->engine());
  }
  if (!bad.empty()) {
    RCLCPP_ERROR_STREAM(kLog, bad << ": no ground plane" << (cfg_.obstacles ? ", the obstacle stage keeps its file's mount" : ""));
    return;
  }
  cfg_.ground = true;
  RCLCPP_WARN_STREAM(kLog, "ground: " << p.hypotheses << " hypotheses, " << p.refits << " refits, tol " << p.tol_px << " px"
                                      << (cfg_.obstacles ? ", the obstacle stage takes every frame's mount" : ""));
}

// the frame's ground plane; logs height and tilt when either moved by more than log_delta since the last line
bool StereonetNode::FitGround(const int32_t* raw, sn_ground* g) {
  if (sn_ground_from_raw(net_->engine(), 1, raw, &cfg_.camera, &cfg_.ground_params, g, nullptr, SN_MEM_HOST, nullptr) != SN_OK) {
    RCLCPP_ERROR(kLog, "ground failed: %s", sn_last_error(net_->engine()));
    return false;
  }
  const float* m = g->base_from_cam;
  const float hgt = m[11], pitch = std::asin(std::max(-1.f, std::min(1.f, -m[10]))), roll = std::asin(std::max(-1.f, std::min(1.f, -m[8])));
  const float d = cfg_.ground_log_delta;
  if (ground_logged_[0] < 0.f || std::fabs(hgt - ground_logged_[0]) > d || std::fabs(pitch - ground_logged_[1]) > d ||
      std::fabs(roll - ground_logged_[2]) > d) {
    RCLCPP_WARN(kLog, "ground: %s, height %.3f m, pitch %.4f rad, roll %.4f rad, %u inliers of %u",
                (g->flags & SN_GROUND_FOUND) ? "found" : "not found (the prior mount)", hgt, pitch, roll, g->inliers, g->usable);
    ground_logged_[0] = hgt, ground_logged_[1] = pitch, ground_logged_[2] = roll;
  }
  return true;
}

void StereonetNode::LogModelIo() {
  RCLCPP_WARN_STREAM(kLog, "model_input_count: " << net_->GetInputCount() << ", model_input_width: " << net_w_
                                                 << ", model_input_height: " << net_h_);
  hbDNNTensorProperties p;
  for (int i = 0; i < net_->GetInputCount(); ++i)
    if (hbDNNGetInputTensorProperties(&p, net_->GetDNNHandle(), i) == 0)
      RCLCPP_INFO_STREAM(kLog, "input_idx: " << i << ", tensorType = " << p.tensorType << ", tensorLayout = "
                                             << p.tensorLayout << ", shape " << p.validShape.dimensionSize[0] << "x"
                                             << p.validShape.dimensionSize[1] << "x" << p.validShape.dimensionSize[2]
                                             << "x" << p.validShape.dimensionSize[3]);
  for (int i = 0; i < net_->GetOutputCount(); ++i)
    if (hbDNNGetOutputTensorProperties(&p, net_->GetDNNHandle(), i) == 0)
      RCLCPP_WARN_STREAM(kLog, "output_idx: " << i << ", tensorType = " << p.tensorType
                                              << ", tensorLayout = " << p.tensorLayout);
}

int StereonetNode::SetNodePara() {
  if (!dnn_node_para_ptr_) return -1;
  if (access(cfg_.model_file.c_str(), F_OK) != 0) {
    RCLCPP_ERROR_STREAM(rclcpp::get_logger("hobot_stereonet"), "File is not exist! model_file: " << cfg_.model_file);
    return -1;
  }
  dnn_node_para_ptr_->model_file = cfg_.model_file;
  dnn_node_para_ptr_->model_task_type = hobot::dnn_node::ModelTaskType::ModelInferType;
  dnn_node_para_ptr_->task_num = 4;   // requests in flight
  return 0;
}

namespace {
// STEREONET_JPEG=gpu: the frame's stream by ONE pool task that calls sn_jpeg_encode_nv12 (host mode: the call stages the frame
// and blocks the pool thread, not FeedImg), with the rows_per_slice of SubmitSlicedJpeg, so the bytes are those of the host
// encoder.  A failed call or a stream that did not fit completes the future with false: the jpeg_bad path of PostProcess.
std::shared_future<bool> SubmitGpuJpeg(JpegPool& pool, sn_handle* engine, std::shared_ptr<const void> keep_alive, const uint8_t* nv12,
                                       int w, int h, int pitch, int quality, int slices, std::shared_ptr<BinDataType> out) {
  const int rows = JpegMcuRows(h);
  int nsl = slices < 1 ? 1 : slices;
  if (nsl > rows) nsl = rows;
  const int per = (rows + nsl - 1) / nsl;
  nsl = (rows + per - 1) / per;
  auto done = std::make_shared<std::promise<bool>>();
  std::shared_future<bool> fut = done->get_future().share();
  pool.Post([engine, keep_alive, nv12, out, done, w, h, pitch, quality, per, nsl] {
    static thread_local std::vector<uint8_t> stream;      // sn_jpeg_bound bytes, once per thread: no 9 MB vector per frame
    const size_t cap = sn_jpeg_bound(w, h);
    if (stream.size() < cap) stream.resize(cap);
    const sn_jpeg_params p{quality, nsl > 1 ? per : 0};
    uint32_t size = 0;
    const int rc = sn_jpeg_encode_nv12(engine, 1, nv12, w, h, pitch, 0, &p, stream.data(), stream.size(), &size, SN_MEM_HOST, nullptr);
    const bool ok = rc == SN_OK && size != 0;
    if (ok) out->jpeg.assign(stream.begin(), stream.begin() + size);
    else out->jpeg.clear();
    done->set_value(ok);
  });
  return fut;
}
}  // namespace

void StereonetNode::OnStereoFrame(const hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr received) {
  if (!rclcpp::ok() || !received) return;
  hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr frame = received;

  // accept only NV12 frames that hold both eyes side by side at the model's resolution
  const char* enc = reinterpret_cast<const char*>(frame->encoding.data());
  if (strncmp(enc, "nv12", frame->encoding.size()) != 0) {
    RCLCPP_ERROR(kLog, "Only support nv12 img encoding!");
    return;
  }
  if (rectify_ && !(frame = RectifyFrame(received))) return;
  if ((int)frame->height != net_h_ || (int)frame->width != 2 * net_w_) {
    RCLCPP_ERROR_STREAM(kLog, "recved img msg h: " << frame->height << ", w: " << frame->width
                                                   << " is unmatch with model_input_width: " << net_w_
                                                   << ", model_input_height: " << net_h_);
    return;
  }
  const int w = net_w_, h = net_h_, pitch = 2 * w, rows = h + h / 2;
  if (frame->data.size() < (size_t)pitch * rows) return;

  auto request = std::make_shared<StereonetNodeOutput>();
  request->msg_header = std::make_shared<std_msgs::msg::Header>();
  request->msg_header->frame_id = std::to_string(frame->index);
  request->msg_header->stamp = frame->time_stamp;
  if (cfg_.pointcloud_layout >= 0 || (temporal_ && cfg_.temporal.luma_delta > 0) || cfg_.render) request->frame = frame;

  const auto t_pre = std::chrono::steady_clock::now();
  // STEREONET_INGEST=tensor keeps the reference's host steps (split both eyes, CvtNV12Data2Tensors, Run on the int8
  // tensor); the default hands the message payload to the backend, which does the same byte mapping on the GPU
  // The device ingest reads the frame in 8-byte units (sn_submit_nv12: the side-by-side width must be a multiple of 8,
  // the height even); any other even geometry the reference accepts goes through the host steps, as it does there.
  static const bool want_tensor = getenv("STEREONET_INGEST") != nullptr && !strcmp(getenv("STEREONET_INGEST"), "tensor");
  const bool host_tensor = want_tensor || ((2 * net_w_) & 7) != 0 || (net_h_ & 1) != 0;
  // de-interleave the eyes: every source row carries w bytes of the left eye, then w bytes of the right eye
  const unsigned char* row = frame->data.data();
  if (host_tensor) {
    eye_l_.resize((size_t)w * rows);
    eye_r_.resize((size_t)w * rows);
    for (int r = 0; r < rows; ++r, row += pitch) {
      memcpy(eye_l_.data() + (size_t)r * w, row, w);
      memcpy(eye_r_.data() + (size_t)r * w, row + w, w);
    }
  }
  std::vector<std::shared_ptr<DNNTensor>> tensors;
  if (host_tensor && pre_->CvtNV12Data2Tensors(tensors, net_, eye_l_.data(), eye_r_.data()) < 0) {
    RCLCPP_ERROR(kLog, "Preprocess fail");
    rclcpp::shutdown();
    return;
  }
  if (cfg_.publish_output) {
    // the left eye is the left half of every row of the side-by-side frame: the encoder reads it in place (pitch 2w); the
    // job keeps the message alive, nothing is copied on this thread
    auto left = std::make_shared<BinDataType>();
    left->w = w;
    left->h = h;
    request->sp_left_nv12 = left;
    const int quality = cfg_.jpeg_quality;
    const auto tq = std::chrono::steady_clock::now();
    request->jpeg_ready = cfg_.jpeg_gpu ? SubmitGpuJpeg(*jpeg_pool_, net_->engine(), frame, frame->data.data(), w, h, pitch, quality,
                                                        cfg_.jpeg_slices, left)
                                        : SubmitSlicedJpeg(*jpeg_pool_, frame, frame->data.data(), w, h, pitch, quality,
                                                           cfg_.jpeg_slices, left);
    g_stats.add(1, tq);
  }
  request->preprocess_time_ms = elapsed_ms(t_pre);
  RCLCPP_INFO(kLog, "Preprocess done, time cost %d ms", request->preprocess_time_ms);

  const auto tr = std::chrono::steady_clock::now();
  const int rc = host_tensor ? Run(tensors, request, /*is_sync_mode=*/false, -1, -1)
                             : RunSbsNv12(frame->data.data(), 2 * w, h, request, /*is_sync_mode=*/false, -1);
  g_stats.add(2, tr);
  g_stats.add(0, t_pre);
  if (rc < 0) {
    RCLCPP_ERROR(kLog, "Run infer fail!");
    return;
  }
  RCLCPP_INFO(kLog, "Run infer done");
}

namespace {
// one path per line; every entry must exist (stereonet_node.cpp:832-878)
bool read_list(const std::string& list_file, std::vector<std::string>& out) {
  std::ifstream in(list_file);
  if (!in.good()) {
    RCLCPP_ERROR_STREAM(kLog, "Open file failed: " << list_file);
    return false;
  }
  std::string line;
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (access(line.c_str(), F_OK) != 0) {
      RCLCPP_ERROR_STREAM(kLog, "File is not exist! img_name: " << line);
      return false;
    }
    out.push_back(line);
  }
  return true;
}
}  // namespace

int StereonetNode::RunImglistFeedInfer(std::string left_img_list, std::string right_img_list) {
  if (!rclcpp::ok() || !ready_) return 0;
  RCLCPP_INFO_STREAM(kLog, "Feedback with left_img_list: " << left_img_list << " right_img_list: " << right_img_list);
  std::vector<std::string> left, right;
  if (!read_list(left_img_list, left) || !read_list(right_img_list, right)) {
    rclcpp::shutdown();
    return 0;
  }
  if (left.size() != right.size()) {
    RCLCPP_ERROR_STREAM(kLog, "Imgs size error! left_imgs.size: " << left.size() << ", right_imgs.size: " << right.size());
    rclcpp::shutdown();
    return 0;
  }
  int start_ms = cfg_.feed_start_pause_ms, frame_ms = cfg_.feed_frame_pause_ms;
  if (const char* e = getenv("STEREONET_FEED_PAUSE_MS")) start_ms = frame_ms = atoi(e);
  std::this_thread::sleep_for(std::chrono::milliseconds(start_ms));

  int done = 0;
  std::vector<uint8_t> bgr;
  std::vector<unsigned char> nv12[2];
  for (size_t idx = 0; idx < left.size(); ++idx) {
    RCLCPP_WARN_STREAM(kLog, "Feed " << idx << "/" << left.size());
    if (!rclcpp::ok()) return done;
    const std::string* path[2] = {&left[idx], &right[idx]};
    for (int eye = 0; eye < 2; ++eye) {
      int w = 0, h = 0;
      std::string why;
      if (!ReadImageBGR(*path[eye], w, h, bgr, &why)) {
        RCLCPP_ERROR_STREAM(kLog, "BGRToNv12 Fail: " << why);
        rclcpp::shutdown();
        return done;
      }
      // the reference feeds whatever imread returned; a size other than the model's would read out of bounds
      // there, so it is an error here
      if (w != net_w_ || h != net_h_ || Tools::BGRToNv12(bgr.data(), w, h, nv12[eye]) != 0) {
        RCLCPP_ERROR_STREAM(kLog, "BGRToNv12 Fail: " << *path[eye] << " is " << w << "x" << h << ", model input is "
                                                     << net_w_ << "x" << net_h_);
        rclcpp::shutdown();
        return done;
      }
    }
    auto request = std::make_shared<StereonetNodeOutput>();
    request->msg_header = std::make_shared<std_msgs::msg::Header>();
    request->msg_header->frame_id = std::to_string(idx);
    std::vector<std::shared_ptr<DNNTensor>> tensors;
    if (pre_->CvtNV12Data2Tensors(tensors, net_, nv12[0].data(), nv12[1].data()) < 0) {
      RCLCPP_ERROR(kLog, "Preprocess fail");
      rclcpp::shutdown();
      return done;
    }
    if (cfg_.publish_output) {
      auto jpg = std::make_shared<BinDataType>();
      jpg->w = net_w_;
      jpg->h = net_h_;
      if (!EncodeNv12ToJpeg(nv12[0].data(), net_w_, net_h_, net_w_, cfg_.jpeg_quality, jpg->jpeg)) {
        RCLCPP_ERROR(kLog, "invalid sp_left_nv12");
        rclcpp::shutdown();
        return done;
      }
      request->sp_left_nv12 = jpg;
    }
    if (Run(tensors, request, /*is_sync_mode=*/true, -1, -1) < 0) {
      RCLCPP_ERROR(kLog, "Run infer fail!");
      return done;
    }
    ++done;
    RCLCPP_INFO(kLog, "Run infer done");
    std::this_thread::sleep_for(std::chrono::milliseconds(frame_ms));
  }
  return done;
}

int StereonetNode::PostProcess(const std::shared_ptr<hobot::dnn_node::DnnNodeOutput>& node_output) {
  if (!rclcpp::ok()) return 0;
  auto request = std::dynamic_pointer_cast<StereonetNodeOutput>(node_output);
  if (!request) {
    RCLCPP_ERROR(kLog, "Cast dnn node output fail!");
    return -1;
  }
  const auto t_pub = std::chrono::steady_clock::now();
  int pack_ms = 0;
  const auto tw = std::chrono::steady_clock::now();
  const bool jpeg_bad = cfg_.publish_output && request->sp_left_nv12 && request->jpeg_ready.valid() && !request->jpeg_ready.get();
  g_stats.add(3, tw);
  if (jpeg_bad) {
    RCLCPP_ERROR(kLog, "invalid sp_left_nv12");      // the worker's encode failed (FeedImg's check, stereonet_node.cpp:797)
    rclcpp::shutdown();
    return -1;
  }
  // ahead of the message and of the cloud: both see the filtered map
  if (temporal_ && !request->output_tensors.empty())
    FilterTemporal(*request, static_cast<int32_t*>(request->output_tensors[0]->sysMem[0].virAddr));
  // the view of the filtered map, ahead of the message it belongs to: whoever has the message has the view as well
  if (render_out_ && !request->output_tensors.empty())
    PublishRender(*request, static_cast<const int32_t*>(request->output_tensors[0]->sysMem[0].virAddr));
  if (cfg_.publish_output && request->sp_left_nv12 && !request->output_tensors.empty()) {
    // wire format consumed by the render node: sensor_msgs/Image, encoding "jpeg",
    // data = the raw int32 output tensor followed by the JPEG of the left eye, step = total length
    const hbSysMem& out = request->output_tensors[0]->sysMem[0];
    const std::vector<uint8_t>& jpeg = request->sp_left_nv12->jpeg;
    sensor_msgs::msg::Image msg;
    msg.header = *request->msg_header;
    msg.width = request->sp_left_nv12->w;
    msg.height = request->sp_left_nv12->h;
    msg.encoding = "jpeg";
    // one allocation, two copies, no zero fill (resize() + memcpy wrote the 3.7 MB twice)
    const uint8_t* raw = static_cast<const uint8_t*>(out.virAddr);
    msg.data.reserve(out.memSize + jpeg.size());
    msg.data.insert(msg.data.end(), raw, raw + out.memSize);
    msg.data.insert(msg.data.end(), jpeg.begin(), jpeg.end());
    msg.step = (uint32_t)msg.data.size();
    pack_ms = elapsed_ms(t_pub);
    RCLCPP_INFO(kLog, "publish output with msg index: %s, topic: %s, time cost ms: %d",
                request->msg_header->frame_id.c_str(), cfg_.output_topic.c_str(), pack_ms);
    g_stats.add(4, t_pub);
    const auto tp = std::chrono::steady_clock::now();
    disparity_out_->publish(std::move(msg));
    g_stats.add(5, tp);
  } else {
    RCLCPP_INFO(kLog, "publish is unable");
  }
  if (pointcloud_out_ && !request->output_tensors.empty())
    PublishPointCloud(*request, static_cast<const int32_t*>(request->output_tensors[0]->sysMem[0].virAddr));
  if ((cfg_.obstacles || cfg_.ground || elevation_) && !request->output_tensors.empty()) {
    const int32_t* raw = static_cast<const int32_t*>(request->output_tensors[0]->sysMem[0].virAddr);
    sn_ground g;
    const bool fitted = cfg_.ground && FitGround(raw, &g);
    if (cfg_.obstacles) PublishObstacles(*request, raw, fitted ? g.base_from_cam : nullptr);
    if (elevation_) PublishElevation(*request, raw, fitted ? g.base_from_cam : nullptr);
  }
  const auto& st = node_output->rt_stat;
  if (st && st->fps_updated)
    RCLCPP_WARN(kLog,
                "input fps: %.2f, out fps: %.2f, preprocess time ms: %d, infer time ms: %d, msg preparation for pub "
                "time cost ms: %d, refinement residual px: %.3f, arithmetic: %s",
                st->input_fps, st->output_fps, request->preprocess_time_ms, st->infer_time_ms, pack_ms,
                st->refine_residual_px, st->arithmetic);
  return 0;
}

}  // namespace stereonet
}  // namespace hobot
