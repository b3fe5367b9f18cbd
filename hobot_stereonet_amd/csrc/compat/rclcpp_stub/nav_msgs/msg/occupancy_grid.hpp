// Shape of nav_msgs/msg/OccupancyGrid (member names of the real message, so the node builds against ROS 2 unchanged).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>
#include "nav_msgs/msg/map_meta_data.hpp"
#include "std_msgs/msg/header.hpp"
namespace nav_msgs { namespace msg {
struct OccupancyGrid {
  using SharedPtr = std::shared_ptr<OccupancyGrid>;
  using ConstSharedPtr = std::shared_ptr<const OccupancyGrid>;
  std_msgs::msg::Header header;
  MapMetaData info;
  std::vector<int8_t> data;               // row-major, index iy * width + ix: 0..100 occupancy, -1 unknown
};
}}
