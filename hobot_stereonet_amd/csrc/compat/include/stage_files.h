// stage_files.h — the node's stage files: for each stage the keys of its file (read by param_file.h's reader) and the values a
// file that names no key leaves in place, which are the defaults of the Python dataclass that writes the file
// (tests/test_param_files.py holds the two together).  Needs the structs of stereonet_hip.h and no engine symbol.
#pragma once

#include <string>
#include <vector>

#include "stereonet_hip.h"

namespace hobot {
namespace stereonet {

constexpr const char* kDefaultBaseFrame = "base_link";      // obstacles.ObstacleParams.frame
constexpr const char* kDefaultFixedFrame = "odom";          // costmap.CostmapParams.frame, elevation.ElevationParams.frame
constexpr float kDefaultGroundLogDelta = 0.02f;             // ground.GroundParams.log_delta

sn_obstacle_params default_obstacle_params();
sn_ground_params default_ground_params();
sn_costmap_params default_costmap_params();
sn_elevation_params default_elevation_params();
sn_inflate_params default_inflate_params();
sn_nav_params default_plan_params();
sn_rollout_params default_rollout_params();

// false: *err says why, without the file's name.  The calibration needs every key; elsewhere a key that is missing keeps what
// *p (and the side outputs) held
bool load_calib_file(const char* path, sn_stereo_calib* c, std::string* err);
bool load_obstacle_file(const char* path, sn_obstacle_params* p, std::string* frame, std::string* err);
bool load_ground_file(const char* path, sn_ground_params* p, float* log_delta, std::string* err);
bool load_costmap_file(const char* path, sn_costmap_params* p, std::string* frame, std::string* err);
bool load_elevation_file(const char* path, sn_elevation_params* p, std::string* frame, bool* feed_inflate, std::string* err);
bool load_inflate_file(const char* path, sn_inflate_params* p, std::string* err);
bool load_plan_file(const char* path, sn_nav_params* p, std::string* err);
bool load_rollout_file(const char* path, sn_rollout_params* p, std::vector<float>* footprint, double* acc, bool* has_acc, std::string* err);

}  // namespace stereonet
}  // namespace hobot
