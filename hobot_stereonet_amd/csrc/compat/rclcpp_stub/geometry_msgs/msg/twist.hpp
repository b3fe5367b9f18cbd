// Shape of geometry_msgs/msg/Twist with its Vector3 (member names of the real messages).
#pragma once
#include <memory>
namespace geometry_msgs { namespace msg {
struct Vector3 {
  double x = 0.0, y = 0.0, z = 0.0;
};
struct Twist {
  using SharedPtr = std::shared_ptr<Twist>;
  using ConstSharedPtr = std::shared_ptr<const Twist>;
  Vector3 linear;       // m/s; a differential drive uses x
  Vector3 angular;      // rad/s; ... and z
};
}}
