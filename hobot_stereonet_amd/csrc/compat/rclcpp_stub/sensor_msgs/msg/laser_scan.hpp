// Shape of sensor_msgs/msg/LaserScan (member names of the real message, so the node builds against ROS 2 unchanged).
#pragma once
#include <memory>
#include <vector>
#include "std_msgs/msg/header.hpp"
namespace sensor_msgs { namespace msg {
struct LaserScan {
  using SharedPtr = std::shared_ptr<LaserScan>;
  using ConstSharedPtr = std::shared_ptr<const LaserScan>;
  std_msgs::msg::Header header;
  float angle_min = 0.f, angle_max = 0.f, angle_increment = 0.f;
  float time_increment = 0.f, scan_time = 0.f;
  float range_min = 0.f, range_max = 0.f;
  std::vector<float> ranges, intensities;
};
}}
