// stereonet_node.h — the ROS 2 node of this repo's host mirror.
//
// Public contract kept identical to the reference node so that launch files and downstream nodes need no
// change (reference: stereonet_infer/include/stereonet_node.h:61-71 for the class surface, :97,:106,:120-121
// for the parameter defaults):
//   class hobot::stereonet::StereonetNode : public hobot::dnn_node::DnnNode
//   StereonetNode(node_name = "stereonet_node", options)
//   overrides SetNodePara() / PostProcess(output)
//   parameters config_file, model_file, sub_hbmem_topic_name, ros_img_topic_name
// Everything private is this implementation's own: settings are grouped in one struct, per-frame scratch is
// reused across frames, and the inference behind DnnNode::Run is libstereonet_hip.so.
#pragma once

#include <atomic>
#include <cstdint>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include <mutex>

#include "rclcpp/rclcpp.hpp"
#include "nav_msgs/msg/occupancy_grid.hpp"
#include "nav_msgs/msg/path.hpp"
#include "geometry_msgs/msg/twist.hpp"
#include "sensor_msgs/msg/image.hpp"
#include "sensor_msgs/msg/laser_scan.hpp"
#include "sensor_msgs/msg/point_cloud2.hpp"
#include "ai_msgs/msg/perception_targets.hpp"
#include "hbm_img_msgs/msg/hbm_msg1080_p.hpp"

#include "dnn_node/dnn_node.h"
#include "stereonet_hip.h"
#include "bin_data.h"
#include "preprocess.h"
#include "stage_files.h"

namespace hobot {
namespace stereonet {

// Per-request context handed through DnnNode::Run.
struct StereonetNodeOutput : public hobot::dnn_node::DnnNodeOutput {
  std::shared_ptr<BinDataType> sp_left_nv12;
  int preprocess_time_ms = 0;
  // this implementation's own: set when the left-eye JPEG of this request is being encoded on a worker thread
  // (sp_left_nv12->jpeg is complete once it yields true); PostProcess waits for it
  std::shared_future<bool> jpeg_ready;
  // kept only while the point cloud is on (STEREONET_POINTCLOUD), the temporal filter reads the luma (STEREONET_TEMPORAL
  // with LUMA_DELTA > 0) or the depth view is on (STEREONET_RENDER): the frame whose left eye colours the cloud, guides the
  // filter and tops the view
  hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr frame;
};

class JpegPool;      // worker threads that encode the left-eye JPEGs of requests in flight (stereonet_node.cpp)

class StereonetNode : public hobot::dnn_node::DnnNode {
 public:
  StereonetNode(const std::string& node_name = "stereonet_node",
                const rclcpp::NodeOptions& options = rclcpp::NodeOptions());
  ~StereonetNode() override;

  // true once the model is loaded and the subscription exists (the harness checks it; the reference shuts
  // rclcpp down instead, which this node does as well)
  bool IsReady() const { return ready_; }

  // Offline feeder (reference: stereonet_node.h:118, stereonet_node.cpp:820-976, disabled in its constructor):
  // two text files with one image path per line; frame i = (left[i], right[i]) -> BGR -> NV12 -> model tensor,
  // synchronous Run with frame_id = i, result published like a live frame.  Any unreadable list or image, a
  // length mismatch, or an image that is not the model's size ends the run with rclcpp::shutdown(), as the
  // reference does.  Returns the number of frames that went through PostProcess.
  int RunImglistFeedInfer(std::string left_img_list, std::string right_img_list);

  // this implementation's own: the robot's planar pose in the costmap's fixed frame (metres, radians), taken by every frame
  // processed after the call (STEREONET_COSTMAP).  Thread-safe; the default is the origin.
  void SetBasePose(double x, double y, double yaw);

  // this implementation's own: the goal of the plan (STEREONET_PLAN), metres in the frame of the inflated grid's source (the
  // costmap's fixed frame when the costmap is on), taken by every frame processed after the call.  Thread-safe; until the first
  // call nothing is published on /stereonet_plan.
  void SetGoal(double x_m, double y_m);

  // this implementation's own: the robot's present velocity (m/s, rad/s) for the rollout (STEREONET_ROLLOUT), taken by every
  // frame processed after the call: with the file's `acc` line it narrows the samples to those the motors reach (the window of
  // sn_rollout).  Thread-safe; until the first call, or without an `acc` line, every sample is admitted.
  void SetVelocity(double v, double w);

 protected:
  int SetNodePara() override;
  int PostProcess(const std::shared_ptr<hobot::dnn_node::DnnNodeOutput>& node_output) override;

 private:
  struct Settings {
    std::string config_file = "config/hobot_stereonet_config.json";   // declared, never opened (as in the reference)
    std::string model_file = "config/hobot_stereonet.hbm";
    std::string image_topic = "hbmem_stereo_img";
    std::string output_topic = "/stereonet_node_output";
    bool publish_output = true;       // the reference's enable_pub_output_ (a constant there); STEREONET_PUB_OUTPUT=0 turns it off
    int jpeg_quality = 95;
    int jpeg_threads = 0;             // 0 = hardware threads / 4, clamped to 2..32; STEREONET_JPEG_THREADS overrides
    int jpeg_slices = 8;              // restart-interval slices per frame, encoded in parallel (1 = one scan, no RSTm);
                                      // STEREONET_JPEG_SLICES overrides
    bool jpeg_gpu = false;            // STEREONET_JPEG=gpu: the encoder task is one sn_jpeg_encode_nv12 call per frame instead of
                                      // jpeg_slices host tasks; the stream is the same bytes (default: host)
    int feed_start_pause_ms = 1000;   // the reference waits for the viewer before / between offline frames
    int feed_frame_pause_ms = 300;    // (stereonet_node.cpp:890,974); STEREONET_FEED_PAUSE_MS overrides both
    // this implementation's own: sensor_msgs/PointCloud2 on /stereonet_pointcloud2 (sn_pointcloud_from_raw).
    // STEREONET_POINTCLOUD=organised|compact turns it on (unset: off, nothing of it exists);
    // STEREONET_CAMERA=fx,fy,cx,cy,baseline_mm (cx, cy default to the map's centre), STEREONET_POINTCLOUD_STEP=1|2|4,
    // STEREONET_POINTCLOUD_Z=min,max (metres; max <= 0: no upper bound)
    int pointcloud_layout = -1;       // -1 off, else SN_PC_ORGANISED / SN_PC_COMPACT
    sn_camera camera{};
    // this implementation's own: the temporal filter of the disparity stream (sn_temporal_push), applied to the int32 tensor
    // in place before it is packed and before the cloud is built.  STEREONET_TEMPORAL=ALPHA,DELTA_PX[,PERSIST[,LUMA_DELTA]]
    // (PERSIST defaults to 2, LUMA_DELTA to 0) turns it on; unset: off, nothing of it exists
    sn_temporal_params temporal{};
    // this implementation's own: rectification of RAW frames ahead of everything else (sn_rectify_nv12).
    // STEREONET_RECTIFY=<calibration file> (size, left.K / .D / .R, right.K / .D / .R, P, baseline_mm: one `key v v ...` per
    // line, `#` comments) turns it on; unset: off, nothing of it exists
    sn_stereo_calib calib{};
    // this implementation's own: the reference render node's picture (colour-mapped depth under the left eye) as
    // sensor_msgs/Image "jpeg" on /image_jpeg, one sn_render_jpeg call per frame on the map after the temporal filter.
    // STEREONET_RENDER=Q[,ROWS] (JPEG quality, MCU rows per restart interval; ROWS defaults to 1) turns it on, with
    // STEREONET_RENDER_TRUE=1 (the colour map's own colours) and STEREONET_RENDER_INVALID_BLACK=1; unset: off, nothing of it exists
    bool render = false;
    sn_render_params render_params{};
    sn_jpeg_params render_jpeg{95, 1};
    // this implementation's own: where the robot cannot drive (sn_obstacles_from_raw), from the map the point cloud gets:
    // nav_msgs/OccupancyGrid on /stereonet_obstacle_grid and sensor_msgs/LaserScan on /stereonet_scan, whichever of the two
    // the file configures.  STEREONET_OBSTACLES=<parameter file> (obstacles.save_params' `key value` lines, `frame` = the frame
    // id, default base_link) turns it on, with the point cloud's camera (STEREONET_CAMERA, STEREONET_POINTCLOUD_STEP / _Z or the
    // rectifier's); unset: off, nothing of it exists
    bool obstacles = false;
    sn_obstacle_params obstacle_params{};
    std::string obstacle_frame = kDefaultBaseFrame;
    // this implementation's own: the ground plane of every frame's map (sn_ground_from_raw) ahead of the obstacle stage, which
    // then classifies with the frame's mount (sn_obstacles_from_raw_mounts) instead of the obstacle file's base_from_cam.
    // STEREONET_GROUND=<parameter file> (ground.save_params' `key value` lines) turns it on, with the camera of the point cloud
    // and the obstacle stage; height and tilt are logged when they change by more than the file's log_delta; unset: off
    bool ground = false;
    sn_ground_params ground_params{};
    float ground_log_delta = kDefaultGroundLogDelta;
    // this implementation's own: a rolling log-odds costmap with ray clearing (sn_costmap_push) over the obstacle stage's grid and
    // scan, at the pose of SetBasePose: nav_msgs/OccupancyGrid on /stereonet_costmap, published after the obstacle topics.
    // STEREONET_COSTMAP=<parameter file> (costmap.save_params' `key value` lines, `frame` = the fixed frame's id, default odom)
    // turns it on and requires STEREONET_OBSTACLES; unset: off, nothing of it exists
    sn_costmap_params costmap_params{};
    std::string costmap_frame = kDefaultFixedFrame;
    // this implementation's own: a rolling elevation map with a step-height traversability verdict (sn_elevation_push) from the
    // request's map at the pose of SetBasePose, with the frame's fitted mount while STEREONET_GROUND is on: the verdict as
    // nav_msgs/OccupancyGrid on /stereonet_traversability, published after the obstacle topics (and the costmap's).
    // STEREONET_ELEVATION=<parameter file> (elevation.save_params' `key value` lines, `frame` = the fixed frame's id, default
    // odom) turns it on; it needs no STEREONET_OBSTACLES.  The file's line `feed_inflate 1` makes this grid the source of
    // /stereonet_inflated_grid (and so of the plan and the rollout) in the place of the costmap's or the obstacle grid;
    // without that line, or unset: nothing the node published before changes
    sn_elevation_params elevation_params{};
    std::string elevation_frame = kDefaultFixedFrame;
    bool elevation_feeds_inflate = false;
    // this implementation's own: inflation by the robot's radius (sn_inflate_grid) of the grid a planner reads: nav_msgs/
    // OccupancyGrid on /stereonet_inflated_grid with the header and info of its source, published right after it: the costmap's
    // grid when the costmap is on, else the obstacle grid.  STEREONET_INFLATE=<parameter file> (inflate.save_params' `key value`
    // lines; cell_m is the source grid's, whatever the file says) turns it on and requires STEREONET_OBSTACLES with a grid;
    // unset: off, nothing of it exists
    bool inflate = false;
    sn_inflate_params inflate_params{};
    // this implementation's own: the navigation function over the inflated costs and the path that follows it (sn_navfn) from
    // the robot's cell (the cell of SetBasePose in the costmap, of the base frame's origin in the obstacle grid) to the goal of
    // SetGoal: nav_msgs/Path on /stereonet_plan, published right after /stereonet_inflated_grid with the header of its source,
    // one pose per cell at the cell's centre in metres, start first.  A goal or a robot outside the grid is clamped to it per
    // coordinate (a goal outside is logged once).  max_path must be 1..2^20.  STEREONET_PLAN=<parameter file> (navfn.save_params' `key value` lines; its
    // goal and start lines are the tools') turns it on and requires STEREONET_INFLATE; unset: off, nothing of it exists
    bool plan = false;
    sn_nav_params plan_params{};
    // this implementation's own: the trajectory rollout (sn_rollout) over the inflated costs and the plan's potential from the
    // robot's pose (SetBasePose in the costmap, the base frame's origin at yaw 0 in the obstacle grid): the best sample's velocity
    // as geometry_msgs/Twist on /stereonet_cmd_vel (linear.x, angular.z; all zero without a valid sample) and its arc as
    // nav_msgs/Path on /stereonet_local_plan (a pose per step in metres with the heading about z; empty without a valid sample),
    // both right after /stereonet_plan with its header, so nothing before the first SetGoal.  STEREONET_ROLLOUT=<parameter file>
    // (rollout.save_params' `key value` lines with its `point x y` footprint lines and the `acc acc_v acc_w dt` line of the
    // window; cell_m is the source grid's, whatever the file says; the `pose` line is the tools') turns it on and requires
    // STEREONET_PLAN; unset: off, nothing of it exists
    bool rollout = false;
    sn_rollout_params rollout_params{};
    std::vector<float> rollout_footprint;         // [nf][2]
    double rollout_acc[3] = {0.0, 0.0, 0.0};      // acc_v, acc_w, dt of the `acc` line
    bool rollout_has_acc = false;
  };

  void DeclareAndReadParameters();
  void LogModelIo();
  void OnStereoFrame(const hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr frame);   // the FeedImg role
  bool ReadCamera(std::string* bad);
  void ReadPointCloudSettings();
  void ReadObstacleSettings();
  void PublishObstacles(const StereonetNodeOutput& request, const int32_t* raw, const float* mount);
  void ReadGroundSettings();
  void ReadCostmapSettings();
  void PublishCostmap(const StereonetNodeOutput& request, const int8_t* occ, const float* ranges);
  void ReadElevationSettings();
  void PublishElevation(const StereonetNodeOutput& request, const int32_t* raw, const float* mount);
  void ReadInflateSettings();
  void PublishInflated(const nav_msgs::msg::OccupancyGrid& src);
  void ReadPlanSettings();
  void PublishPlan(const nav_msgs::msg::OccupancyGrid& src, const uint8_t* cost);
  void ReadRolloutSettings();
  void PublishRollout(const nav_msgs::msg::OccupancyGrid& src, const uint8_t* cost, const uint32_t* potential);
  bool FitGround(const int32_t* raw, sn_ground* out);
  void PublishPointCloud(const StereonetNodeOutput& request, const int32_t* raw);
  void ReadTemporalSettings();
  void ReadRectifySettings();
  hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr RectifyFrame(const hbm_img_msgs::msg::HbmMsg1080P::ConstSharedPtr& raw);
  bool HasModelFrame(const StereonetNodeOutput& request) const;
  void FilterTemporal(const StereonetNodeOutput& request, int32_t* raw);
  void ReadRenderSettings();
  void PublishRender(const StereonetNodeOutput& request, const int32_t* raw);

  Settings cfg_;
  bool ready_ = false;
  int net_w_ = -1, net_h_ = -1;
  hobot::dnn_node::Model* net_ = nullptr;
  std::unique_ptr<PreProcess> pre_;
  std::vector<unsigned char> eye_l_, eye_r_;     // split NV12 eyes, reused across frames
  std::shared_ptr<JpegPool> jpeg_pool_;          // live path: the left eye is encoded off the executor thread

  rclcpp::Subscription<hbm_img_msgs::msg::HbmMsg1080P>::ConstSharedPtr frames_in_;
  rclcpp::Publisher<sensor_msgs::msg::Image>::SharedPtr disparity_out_;
  rclcpp::Publisher<ai_msgs::msg::PerceptionTargets>::SharedPtr targets_out_;   // created for parity, never used
  rclcpp::Publisher<sensor_msgs::msg::PointCloud2>::SharedPtr pointcloud_out_;   // only while the cloud is on
  std::atomic<bool> cloud_uncoloured_logged_{false};
  rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>::SharedPtr obstacle_grid_out_;   // only while STEREONET_OBSTACLES configures a grid
  rclcpp::Publisher<sensor_msgs::msg::LaserScan>::SharedPtr obstacle_scan_out_;    // ... a scan
  float ground_logged_[3] = {-1.f, 0.f, 0.f};     // height, pitch, roll of the last log line; PostProcess only
  sn_temporal* temporal_ = nullptr;              // one stream; only while STEREONET_TEMPORAL is set and valid
  bool temporal_unguided_logged_ = false;        // PostProcess only (one thread at a time)
  rclcpp::Publisher<sensor_msgs::msg::Image>::SharedPtr render_out_;   // only while STEREONET_RENDER is set and valid
  std::atomic<bool> render_no_frame_logged_{false};
  sn_costmap* costmap_ = nullptr;                // one stream; only while STEREONET_COSTMAP is set and valid
  rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>::SharedPtr costmap_out_;
  sn_elevation* elevation_ = nullptr;            // one stream; only while STEREONET_ELEVATION is set and valid
  rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>::SharedPtr traversability_out_;
  rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>::SharedPtr inflated_out_;      // only while STEREONET_INFLATE is set and valid
  rclcpp::Publisher<nav_msgs::msg::Path>::SharedPtr plan_out_;                    // only while STEREONET_PLAN is set and valid
  double goal_[2] = {0.0, 0.0};                  // of SetGoal, under base_pose_mu_
  bool has_goal_ = false;
  std::atomic<bool> goal_clamp_logged_{false};
  rclcpp::Publisher<geometry_msgs::msg::Twist>::SharedPtr cmd_vel_out_;           // only while STEREONET_ROLLOUT is set and valid
  rclcpp::Publisher<nav_msgs::msg::Path>::SharedPtr local_plan_out_;
  double velocity_[2] = {0.0, 0.0};              // of SetVelocity, under base_pose_mu_
  bool has_velocity_ = false;
  std::mutex base_pose_mu_;
  double base_pose_[3] = {0.0, 0.0, 0.0};        // x, y, yaw of SetBasePose
  sn_rectify* rectify_ = nullptr;                // only while STEREONET_RECTIFY names a valid calibration
};

}  // namespace stereonet
}  // namespace hobot
