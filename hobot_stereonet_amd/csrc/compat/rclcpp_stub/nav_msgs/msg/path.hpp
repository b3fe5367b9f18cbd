// Shape of nav_msgs/msg/Path (member names of the real message, so the node builds against ROS 2 unchanged).
#pragma once
#include <memory>
#include <vector>
#include "geometry_msgs/msg/pose_stamped.hpp"
#include "std_msgs/msg/header.hpp"
namespace nav_msgs { namespace msg {
struct Path {
  using SharedPtr = std::shared_ptr<Path>;
  using ConstSharedPtr = std::shared_ptr<const Path>;
  std_msgs::msg::Header header;
  std::vector<geometry_msgs::msg::PoseStamped> poses;      // start first
};
}}
