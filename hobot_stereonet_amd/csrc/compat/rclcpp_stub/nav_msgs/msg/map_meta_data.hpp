// Shape of nav_msgs/msg/MapMetaData (member names of the real message).
#pragma once
#include <cstdint>
#include <memory>
#include "builtin_interfaces/msg/time.hpp"
#include "geometry_msgs/msg/pose.hpp"
namespace nav_msgs { namespace msg {
struct MapMetaData {
  using SharedPtr = std::shared_ptr<MapMetaData>;
  builtin_interfaces::msg::Time map_load_time;
  float resolution = 0.f;                 // metres per cell
  uint32_t width = 0, height = 0;         // cells along x and y
  geometry_msgs::msg::Pose origin;        // the pose of cell (0, 0) in the frame of the header
};
}}
