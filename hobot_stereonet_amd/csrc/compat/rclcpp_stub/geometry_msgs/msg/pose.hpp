// Shape of geometry_msgs/msg/Pose with its Point and Quaternion (member names of the real messages).
#pragma once
#include <memory>
namespace geometry_msgs { namespace msg {
struct Point {
  double x = 0.0, y = 0.0, z = 0.0;
};
struct Quaternion {
  double x = 0.0, y = 0.0, z = 0.0, w = 1.0;
};
struct Pose {
  using SharedPtr = std::shared_ptr<Pose>;
  Point position;
  Quaternion orientation;
};
}}
