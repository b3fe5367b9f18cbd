// stage_files.cpp — one table of keys per stage file, and the defaults beside them
#include "stage_files.h"

#include "param_file.h"

namespace hobot {
namespace stereonet {

// rectify.save_calib's file: every key exactly once.  Whatever is wrong with a line, the message names the whole form
bool load_calib_file(const char* path, sn_stereo_calib* c, std::string* err) {
  double size[2] = {0, 0}, kl[4] = {}, kr[4] = {}, proj[4] = {};
  const bool read = read_param_file(path, {{"size", size, 2},          {"left.K", kl, 4},           {"left.D", c->left.d, 5},
                                           {"left.R", c->left.R, 9},   {"right.K", kr, 4},          {"right.D", c->right.d, 5},
                                           {"right.R", c->right.R, 9}, {"P", proj, 4},              {"baseline_mm", &c->baseline_mm}},
                                    true, err);
  if (!read) {
    if (err->compare(0, 5, "line ") == 0)
      *err = err->substr(0, err->find(':')) + " is not one of size, left.K/.D/.R, right.K/.D/.R, P, baseline_mm with its values";
    return false;
  }
  c->left.fx = kl[0], c->left.fy = kl[1], c->left.cx = kl[2], c->left.cy = kl[3];
  c->right.fx = kr[0], c->right.fy = kr[1], c->right.cx = kr[2], c->right.cy = kr[3];
  c->pfx = proj[0], c->pfy = proj[1], c->pcx = proj[2], c->pcy = proj[3];
  if (!is_int32(size[0]) || !is_int32(size[1])) {
    *err = "size is not two integers";
    return false;
  }
  c->src_w = (int)size[0];
  c->src_h = (int)size[1];
  return true;
}

// obstacles.ObstacleParams: a 10 m x 10 m grid of 0.1 m cells ahead of a level camera, no scan
sn_obstacle_params default_obstacle_params() {
  sn_obstacle_params p{};
  p.y_min_m = -5.f, p.cell_m = 0.1f, p.gw = p.gh = 100;
  p.z_floor_m = -0.15f, p.z_lo_m = 0.1f, p.z_hi_m = 1.5f, p.min_obstacle_hits = p.min_ground_hits = 3;
  return p;
}

bool load_obstacle_file(const char* path, sn_obstacle_params* p, std::string* frame, std::string* err) {
  return read_param_file(path,
                         {{"base_from_cam", p->base_from_cam, 12}, {"x_min_m", &p->x_min_m}, {"y_min_m", &p->y_min_m}, {"cell_m", &p->cell_m},
                          {"z_floor_m", &p->z_floor_m}, {"z_lo_m", &p->z_lo_m}, {"z_hi_m", &p->z_hi_m}, {"angle_min_rad", &p->angle_min_rad},
                          {"angle_increment_rad", &p->angle_increment_rad}, {"range_min_m", &p->range_min_m}, {"range_max_m", &p->range_max_m},
                          {"gw", &p->gw}, {"gh", &p->gh}, {"min_obstacle_hits", &p->min_obstacle_hits}, {"min_ground_hits", &p->min_ground_hits},
                          {"beams", &p->beams}, {"frame", frame}},
                         false, err);
}

// ground.GroundParams: the lower half of the image, 256 hypotheses, two refits, a level prior
sn_ground_params default_ground_params() {
  sn_ground_params p{};
  p.hypotheses = 256, p.seed = 1, p.min_area = 64, p.min_inliers = 100, p.refits = 2;
  p.tol_px = 0.1f, p.max_tilt_rad = 0.5f, p.height_min_m = 0.1f, p.height_max_m = 3.0f;
  return p;
}

bool load_ground_file(const char* path, sn_ground_params* p, float* log_delta, std::string* err) {
  return read_param_file(path,
                         {{"base_from_cam", p->base_from_cam, 12}, {"tol_px", &p->tol_px}, {"max_tilt_rad", &p->max_tilt_rad},
                          {"height_min_m", &p->height_min_m}, {"height_max_m", &p->height_max_m}, {"log_delta", log_delta},
                          {"roi_x", &p->roi_x}, {"roi_y", &p->roi_y}, {"roi_w", &p->roi_w}, {"roi_h", &p->roi_h}, {"hypotheses", &p->hypotheses},
                          {"seed", &p->seed}, {"min_area", &p->min_area}, {"min_inliers", &p->min_inliers}, {"refits", &p->refits}},
                         false, err);
}

// costmap.CostmapParams: a 200 x 200 window, five hits to the upper clamp and five misses to the lower
sn_costmap_params default_costmap_params() { return sn_costmap_params{200, 200, 85, 40, -200, 350, 0.1f, 0.f, 0.f}; }

bool load_costmap_file(const char* path, sn_costmap_params* p, std::string* frame, std::string* err) {
  return read_param_file(path,
                         {{"mw", &p->mw}, {"mh", &p->mh}, {"l_hit", &p->l_hit}, {"l_miss", &p->l_miss}, {"l_min", &p->l_min}, {"l_max", &p->l_max},
                          {"clear_margin_m", &p->clear_margin_m}, {"clear_min_m", &p->clear_min_m}, {"clear_max_m", &p->clear_max_m}, {"frame", frame}},
                         false, err);
}

// elevation.ElevationParams
sn_elevation_params default_elevation_params() {
  sn_elevation_params p{};
  p.mw = p.mh = 200, p.cell_m = 0.1f, p.z_min_m = -1.f, p.z_max_m = 1.5f, p.range_max_m = 6.f;
  p.min_points = 3, p.alpha = 128, p.max_step_mm = 60, p.radius = 1;
  return p;
}

// `feed_inflate` is the node's own key
bool load_elevation_file(const char* path, sn_elevation_params* p, std::string* frame, bool* feed_inflate, std::string* err) {
  int feed = 0;
  if (!read_param_file(path,
                       {{"mw", &p->mw}, {"mh", &p->mh}, {"min_points", &p->min_points}, {"alpha", &p->alpha}, {"max_step_mm", &p->max_step_mm},
                        {"radius", &p->radius}, {"flags", &p->flags}, {"cell_m", &p->cell_m}, {"z_min_m", &p->z_min_m}, {"z_max_m", &p->z_max_m},
                        {"range_max_m", &p->range_max_m}, {"base_from_cam", p->base_from_cam, 12}, {"frame", frame}, {"feed_inflate", &feed}},
                       false, err))
    return false;
  if (feed != 0 && feed != 1) {
    *err = "feed_inflate must be 0 or 1";
    return false;
  }
  *feed_inflate = feed == 1;
  return true;
}

// inflate.InflateParams
sn_inflate_params default_inflate_params() { return sn_inflate_params{0.05f, 0.2f, 0.4f, 10.f, 100, 0}; }

bool load_inflate_file(const char* path, sn_inflate_params* p, std::string* err) {
  return read_param_file(path,
                         {{"cell_m", &p->cell_m}, {"inscribed_radius_m", &p->inscribed_radius_m}, {"inflation_radius_m", &p->inflation_radius_m},
                          {"cost_scaling", &p->cost_scaling}, {"lethal_min", &p->lethal_min}, {"flags", &p->flags}},
                         false, err);
}

// navfn.NavParams
sn_nav_params default_plan_params() { return sn_nav_params{50, 253, 0, 0, 0, 4096}; }

// the tools' `goal x y` and `start x y` lines are read past
bool load_plan_file(const char* path, sn_nav_params* p, std::string* err) {
  return read_param_file(path,
                         {{"neutral", &p->neutral}, {"lethal_cost", &p->lethal_cost}, {"unknown_cost", &p->unknown_cost}, {"flags", &p->flags},
                          {"max_rounds", &p->max_rounds}, {"max_path", &p->max_path}, {"goal", ParamKind::kInt, 2}, {"start", ParamKind::kInt, 2}},
                         false, err);
}

// rollout.RolloutParams
sn_rollout_params default_rollout_params() { return sn_rollout_params{0.05f, 0.f, 0.5f, 11, -1.f, 1.f, 21, 1.5f, 15, 254, 253, 0, 0, 1, 1}; }

// `point x y` once per footprint point, `acc acc_v acc_w dt`; the tools' `pose x y yaw` line is read past
bool load_rollout_file(const char* path, sn_rollout_params* p, std::vector<float>* footprint, double* acc, bool* has_acc, std::string* err) {
  return read_param_file(path,
                         {{"cell_m", &p->cell_m}, {"v_min", &p->v_min}, {"v_max", &p->v_max}, {"w_min", &p->w_min}, {"w_max", &p->w_max},
                          {"sim_time_s", &p->sim_time_s}, {"nv", &p->nv}, {"nw", &p->nw}, {"steps", &p->steps}, {"lethal_cost", &p->lethal_cost},
                          {"centre_lethal_cost", &p->centre_lethal_cost}, {"unknown_cost", &p->unknown_cost}, {"flags", &p->flags},
                          {"w_goal", &p->w_goal}, {"w_occ", &p->w_occ}, {"point", footprint, 2}, {"pose", ParamKind::kDouble, 3},
                          {"acc", acc, 3, has_acc}},
                         false, err);
}

}  // namespace stereonet
}  // namespace hobot
