// Shape of geometry_msgs/msg/PoseStamped (member names of the real message).
#pragma once
#include <memory>
#include "geometry_msgs/msg/pose.hpp"
#include "std_msgs/msg/header.hpp"
namespace geometry_msgs { namespace msg {
struct PoseStamped {
  using SharedPtr = std::shared_ptr<PoseStamped>;
  std_msgs::msg::Header header;
  Pose pose;
};
}}
