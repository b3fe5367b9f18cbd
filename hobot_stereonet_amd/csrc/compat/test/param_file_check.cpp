// param_file_check — the parameter-file reader (src/param_file.cpp) and the node's stage tables (src/stage_files.cpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer (make param_file_check).  No GPU, no library.
//   param_file_check                  a table of cases per file kind, among them the files no saver writes; `param_file_check: ok`
//   param_file_check dump KIND FILE   what the node would make of FILE: `error` and the text it would log, or one `key value...`
//                                     line per field with floats as float32 and doubles as float64 bit patterns
//                                     (tests/test_param_files.py reads this against the Python loaders).  With several
//                                     files, a `== FILE` line goes ahead of each
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "param_file.h"
#include "stage_files.h"

using namespace hobot::stereonet;

namespace {

int failures = 0;

#define CHECK(cond, ...)                                          \
  do {                                                            \
    if (!(cond)) {                                                \
      ++failures;                                                 \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);   \
      std::fprintf(stderr, __VA_ARGS__);                          \
      std::fprintf(stderr, "\n");                                 \
    }                                                             \
  } while (0)

// ---- dump ---------------------------------------------------------------------------------------------------------------------
std::string bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  char s[16];
  snprintf(s, sizeof s, " 0x%08x", u);
  return s;
}
std::string bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  char s[24];
  snprintf(s, sizeof s, " 0x%016llx", (unsigned long long)u);
  return s;
}
std::string bits(int v) { return " " + std::to_string(v); }
std::string bits(uint32_t v) { return " " + std::to_string(v); }
template <class T>
std::string row(const char* key, const T* v, size_t n) {
  std::string s = key;
  for (size_t i = 0; i < n; ++i) s += bits(v[i]);
  return s + "\n";
}
#define F(x) row(#x, &p.x, 1)
#define LIST(x) row(#x, p.x, sizeof(p.x) / sizeof(p.x[0]))

// the variable that names the file of each kind, in the order of the kinds below
const char* const kKinds[8] = {"calib", "obstacle", "ground", "costmap", "elevation", "inflate", "plan", "rollout"};
const char* const kEnv[8] = {"STEREONET_RECTIFY",   "STEREONET_OBSTACLES", "STEREONET_GROUND", "STEREONET_COSTMAP",
                             "STEREONET_ELEVATION", "STEREONET_INFLATE",   "STEREONET_PLAN",   "STEREONET_ROLLOUT"};

int kind_of(const std::string& kind) {
  for (int k = 0; k < 8; ++k)
    if (kind == kKinds[k]) return k;
  return -1;
}

// the node's defaults, the file on top of them, the fields in the struct's order and the side outputs after them
std::string dump(int kind, const std::string& path) {
  std::string err, out, frame;
  bool ok = false;
  switch (kind) {
    case 0: {
      sn_stereo_calib p{};
      ok = load_calib_file(path.c_str(), &p, &err);
      out = F(src_w) + F(src_h);
      for (const sn_eye_calib* e : {&p.left, &p.right}) {
        const std::string name = e == &p.left ? "left" : "right";
        const double k[4] = {e->fx, e->fy, e->cx, e->cy};
        out += row((name + ".K").c_str(), k, 4) + row((name + ".D").c_str(), e->d, 5) + row((name + ".R").c_str(), e->R, 9);
      }
      out += F(pfx) + F(pfy) + F(pcx) + F(pcy) + F(baseline_mm);
      break;
    }
    case 1: {
      sn_obstacle_params p = default_obstacle_params();
      frame = kDefaultBaseFrame;
      ok = load_obstacle_file(path.c_str(), &p, &frame, &err);
      out = LIST(base_from_cam) + F(x_min_m) + F(y_min_m) + F(cell_m) + F(gw) + F(gh) + F(z_floor_m) + F(z_lo_m) + F(z_hi_m) + F(min_obstacle_hits) +
            F(min_ground_hits) + F(beams) + F(angle_min_rad) + F(angle_increment_rad) + F(range_min_m) + F(range_max_m) + "frame " + frame + "\n";
      break;
    }
    case 2: {
      sn_ground_params p = default_ground_params();
      float log_delta = kDefaultGroundLogDelta;
      ok = load_ground_file(path.c_str(), &p, &log_delta, &err);
      out = LIST(base_from_cam) + F(roi_x) + F(roi_y) + F(roi_w) + F(roi_h) + F(hypotheses) + F(seed) + F(min_area) + F(min_inliers) + F(refits) +
            F(tol_px) + F(max_tilt_rad) + F(height_min_m) + F(height_max_m) + row("log_delta", &log_delta, 1);
      break;
    }
    case 3: {
      sn_costmap_params p = default_costmap_params();
      frame = kDefaultFixedFrame;
      ok = load_costmap_file(path.c_str(), &p, &frame, &err);
      out = F(mw) + F(mh) + F(l_hit) + F(l_miss) + F(l_min) + F(l_max) + F(clear_margin_m) + F(clear_min_m) + F(clear_max_m) + "frame " + frame + "\n";
      break;
    }
    case 4: {
      sn_elevation_params p = default_elevation_params();
      frame = kDefaultFixedFrame;
      bool feed = false;
      ok = load_elevation_file(path.c_str(), &p, &frame, &feed, &err);
      out = F(mw) + F(mh) + F(cell_m) + LIST(base_from_cam) + F(z_min_m) + F(z_max_m) + F(range_max_m) + F(min_points) + F(alpha) + F(max_step_mm) +
            F(radius) + F(flags) + "frame " + frame + "\nfeed_inflate " + (feed ? "1\n" : "0\n");
      break;
    }
    case 5: {
      sn_inflate_params p = default_inflate_params();
      ok = load_inflate_file(path.c_str(), &p, &err);
      out = F(cell_m) + F(inscribed_radius_m) + F(inflation_radius_m) + F(cost_scaling) + F(lethal_min) + F(flags);
      break;
    }
    case 6: {
      sn_nav_params p = default_plan_params();
      ok = load_plan_file(path.c_str(), &p, &err);
      out = F(neutral) + F(lethal_cost) + F(unknown_cost) + F(flags) + F(max_rounds) + F(max_path);
      break;
    }
    default: {
      sn_rollout_params p = default_rollout_params();
      std::vector<float> footprint;
      double acc[3] = {0.0, 0.0, 0.0};
      bool has_acc = false;
      ok = load_rollout_file(path.c_str(), &p, &footprint, acc, &has_acc, &err);
      out = F(cell_m) + F(v_min) + F(v_max) + F(nv) + F(w_min) + F(w_max) + F(nw) + F(sim_time_s) + F(steps) + F(lethal_cost) + F(centre_lethal_cost) +
            F(unknown_cost) + F(flags) + F(w_goal) + F(w_occ);
      for (size_t i = 0; i + 1 < footprint.size(); i += 2) out += row("point", &footprint[i], 2);
      if (has_acc) out += row("acc", acc, 3);
    }
  }
  // as Read*Settings logs it: the calibration's message follows the file's name without a colon
  return ok ? out : std::string("error ") + kEnv[kind] + "=" + path + (kind == 0 ? " " : ": ") + err + "\n";
}

// ---- the cases ------------------------------------------------------------------------------------------------------------------
// the keys of each kind as a file spells them: type f float, d double, i int, u uint32, w word, a appends (may repeat)
struct Key {
  const char* name;
  char type;
  int count;
};
const std::vector<Key> kKeys[8] = {
    {{"size", 'd', 2}, {"left.K", 'd', 4}, {"left.D", 'd', 5}, {"left.R", 'd', 9}, {"right.K", 'd', 4}, {"right.D", 'd', 5}, {"right.R", 'd', 9},
     {"P", 'd', 4}, {"baseline_mm", 'd', 1}},
    {{"base_from_cam", 'f', 12}, {"x_min_m", 'f', 1}, {"y_min_m", 'f', 1}, {"cell_m", 'f', 1}, {"z_floor_m", 'f', 1}, {"z_lo_m", 'f', 1},
     {"z_hi_m", 'f', 1}, {"angle_min_rad", 'f', 1}, {"angle_increment_rad", 'f', 1}, {"range_min_m", 'f', 1}, {"range_max_m", 'f', 1}, {"gw", 'i', 1},
     {"gh", 'i', 1}, {"min_obstacle_hits", 'i', 1}, {"min_ground_hits", 'i', 1}, {"beams", 'i', 1}, {"frame", 'w', 1}},
    {{"base_from_cam", 'f', 12}, {"tol_px", 'f', 1}, {"max_tilt_rad", 'f', 1}, {"height_min_m", 'f', 1}, {"height_max_m", 'f', 1}, {"log_delta", 'f', 1},
     {"roi_x", 'i', 1}, {"roi_y", 'i', 1}, {"roi_w", 'i', 1}, {"roi_h", 'i', 1}, {"hypotheses", 'i', 1}, {"seed", 'u', 1}, {"min_area", 'i', 1},
     {"min_inliers", 'i', 1}, {"refits", 'i', 1}},
    {{"mw", 'i', 1}, {"mh", 'i', 1}, {"l_hit", 'i', 1}, {"l_miss", 'i', 1}, {"l_min", 'i', 1}, {"l_max", 'i', 1}, {"clear_margin_m", 'f', 1},
     {"clear_min_m", 'f', 1}, {"clear_max_m", 'f', 1}, {"frame", 'w', 1}},
    {{"mw", 'i', 1}, {"mh", 'i', 1}, {"min_points", 'i', 1}, {"alpha", 'i', 1}, {"max_step_mm", 'i', 1}, {"radius", 'i', 1}, {"flags", 'i', 1},
     {"cell_m", 'f', 1}, {"z_min_m", 'f', 1}, {"z_max_m", 'f', 1}, {"range_max_m", 'f', 1}, {"base_from_cam", 'f', 12}, {"frame", 'w', 1},
     {"feed_inflate", 'i', 1}},
    {{"cell_m", 'f', 1}, {"inscribed_radius_m", 'f', 1}, {"inflation_radius_m", 'f', 1}, {"cost_scaling", 'f', 1}, {"lethal_min", 'i', 1},
     {"flags", 'i', 1}},
    {{"neutral", 'i', 1}, {"lethal_cost", 'i', 1}, {"unknown_cost", 'i', 1}, {"flags", 'i', 1}, {"max_rounds", 'i', 1}, {"max_path", 'i', 1},
     {"goal", 'i', 2}, {"start", 'i', 2}},
    {{"cell_m", 'f', 1}, {"v_min", 'f', 1}, {"v_max", 'f', 1}, {"w_min", 'f', 1}, {"w_max", 'f', 1}, {"sim_time_s", 'f', 1}, {"nv", 'i', 1},
     {"nw", 'i', 1}, {"steps", 'i', 1}, {"lethal_cost", 'i', 1}, {"centre_lethal_cost", 'i', 1}, {"unknown_cost", 'i', 1}, {"flags", 'i', 1},
     {"w_goal", 'i', 1}, {"w_occ", 'i', 1}, {"point", 'a', 2}, {"pose", 'd', 3}, {"acc", 'd', 3}}};

std::string g_dir;
int g_files = 0;

std::string file_of(const std::string& text) {
  const std::string path = g_dir + "/f" + std::to_string(g_files++);
  std::ofstream(path) << text;
  return path;
}

std::string words_of(const Key& k, int count, const std::string& value) {
  std::string s = k.name;
  for (int i = 0; i < count; ++i) s += " " + value;
  return s;
}
std::string line_of(const Key& k, int count, const std::string& value) { return words_of(k, count, value) + "\n"; }

// the whole file of a kind, every key once with 1 for every value, but line `swap` replaced by `with`
std::string file_text(int kind, int swap = -1, const std::string& with = "") {
  std::string s;
  for (size_t i = 0; i < kKeys[kind].size(); ++i) s += (int)i == swap ? with : line_of(kKeys[kind][i], kKeys[kind][i].count, "1");
  return s;
}

// what the dump of `text` must say: "" = accepted, else the reader's message (the calibration's form of it for a line)
void expect(int kind, const std::string& text, int line, const std::string& message, const char* what, const std::string& key) {
  const std::string path = file_of(text), got = dump(kind, path);
  std::string want = message;
  if (line) want = "line " + std::to_string(line) + (kind == 0 ? " is not one of size, left.K/.D/.R, right.K/.D/.R, P, baseline_mm with its values" : ": " + message);
  if (want.empty()) {
    CHECK(got.compare(0, 6, "error ") != 0, "%s %s %s: refused: %s", kKinds[kind], what, key.c_str(), got.c_str());
  } else {
    const std::string full = std::string("error ") + kEnv[kind] + "=" + path + (kind == 0 ? " " : ": ") + want + "\n";
    CHECK(got == full, "%s %s %s: got %s, not %s", kKinds[kind], what, key.c_str(), got.c_str(), full.c_str());
  }
}

bool has_line(const std::string& dumped, const std::string& line) { return ("\n" + dumped).find("\n" + line + "\n") != std::string::npos; }

void cases_of(int kind) {
  const std::vector<Key>& keys = kKeys[kind];
  const int n = (int)keys.size();
  const std::string whole = file_text(kind);
  expect(kind, whole, 0, "", "every key once", "");
  CHECK(dump(kind, g_dir + "/none") == std::string("error ") + kEnv[kind] + "=" + g_dir + "/none" + (kind == 0 ? " " : ": ") + "cannot be opened\n",
        "%s: a missing file", kKinds[kind]);
  if (kind == 0) {
    expect(kind, "", 0, "has no `size` line", "an empty file", "");
    expect(kind, "# nothing\n\n   \n", 0, "has no `size` line", "comments only", "");
  } else {
    const std::string none = dump(kind, file_of(""));
    CHECK(none.compare(0, 6, "error ") != 0, "%s: an empty file refused", kKinds[kind]);
    CHECK(dump(kind, file_of("# nothing\n\n   \n   # more\n")) == none, "%s: comments only", kKinds[kind]);
  }
  // a comment line ahead, blank lines between, a comment after the values: the same struct
  std::string dressed = "# head\n";
  for (int i = 0; i < n; ++i) dressed += "\n  " + words_of(keys[i], keys[i].count, "1") + "   # tail 7\n";
  CHECK(dump(kind, file_of(dressed)) == dump(kind, file_of(whole)), "%s: comments change the outcome", kKinds[kind]);
  expect(kind, whole + "bogus 1\n", n + 1, "unknown key bogus", "an unknown key", "bogus");
  expect(kind, whole + "bogus\n", n + 1, "unknown key bogus", "an unknown key without values", "bogus");
  for (int i = 0; i < n; ++i) {
    const Key& k = keys[i];
    const std::string name = k.name;
    if (k.type == 'a') {
      expect(kind, whole + line_of(k, k.count, "1"), 0, "", "repeated", name);
    } else {
      expect(kind, whole + line_of(k, k.count, "1"), n + 1, name + " twice", "repeated", name);
      expect(kind, whole + line_of(k, k.count, "x"), n + 1, name + " twice", "repeated with a wrong value: `twice` comes first", name);
    }
    expect(kind, file_text(kind, i, line_of(k, k.count - 1, "1")), i + 1, "wrong values for " + name, "too few values", name);
    expect(kind, file_text(kind, i, line_of(k, k.count + 1, "1")), i + 1, "wrong values for " + name, "too many values", name);
    if (kind == 0) expect(kind, file_text(kind, i, ""), 0, "has no `" + name + "` line", "the key missing", name);
    if (k.type == 'w') continue;
    for (const char* bad : {"x", "1x", "--1", "1,5"}) expect(kind, file_text(kind, i, line_of(k, k.count, bad)), i + 1, "wrong values for " + name, bad, name);
    if (k.count > 1)      // a bad value last: the good ones ahead of it are not stored either (below), and the line is refused
      expect(kind, file_text(kind, i, words_of(k, k.count - 1, "1") + " x\n"), i + 1, "wrong values for " + name, "the last value no number", name);
    if (k.type == 'i')
      for (const char* bad : {"1.5", "3e10", "-3e10", "2147483648", "-2147483649", "1e300", "nan", "inf"})
        expect(kind, file_text(kind, i, line_of(k, k.count, bad)), i + 1, "wrong values for " + name, bad, name);
    if (k.type == 'u')
      for (const char* bad : {"1.5", "4294967296", "-1", "3e10", "nan"})
        expect(kind, file_text(kind, i, line_of(k, k.count, bad)), i + 1, "wrong values for " + name, bad, name);
    // the ends of the range are taken and arrive whole (`goal` and `start` are read past: taken is all there is to see)
    if (k.type == 'i' && k.count == 1 && name != "feed_inflate")
      for (const char* edge : {"2147483647", "-2147483648", "2147483647.0", "1e3"}) {
        const std::string got = dump(kind, file_of(line_of(k, 1, edge)));
        CHECK(has_line(got, name + " " + std::to_string((int)strtod(edge, nullptr))), "%s %s %s: %s", kKinds[kind], k.name, edge, got.c_str());
      }
    if (k.type == 'u') CHECK(has_line(dump(kind, file_of(line_of(k, 1, "4294967295"))), name + " 4294967295"), "%s %s at its upper end", kKinds[kind], k.name);
  }
}

// a refused value leaves its destination as it was, whatever its kind, and so does a refused line of several values
void refused_values_store_nothing() {
  sn_obstacle_params o = default_obstacle_params(), o0 = o;
  std::string frame = "keep", err;
  for (const char* text : {"gw 3e10\n", "gw x\n", "gw 1 2\n", "cell_m x\n", "cell_m 1 2\n", "frame a b\n", "base_from_cam 1 2 3 4 5 6 7 8 9 10 11 x\n",
                           "base_from_cam 1 2 3 4 5 6 7 8 9 10 11\n", "gw 7\ngw 8\n"}) {
    o = o0;
    CHECK(!load_obstacle_file(file_of(text).c_str(), &o, &frame, &err), "%s accepted", text);
    if (!strcmp(text, "gw 7\ngw 8\n")) {
      CHECK(o.gw == 7, "the first gw line was not stored");
      o.gw = o0.gw;
    }
    CHECK(!memcmp(&o, &o0, sizeof o) && frame == "keep", "%s stored something", text);
  }
  sn_ground_params g = default_ground_params(), g0 = g;
  float log_delta = 9.f;
  for (const char* text : {"seed -1\n", "seed 4294967296\n", "seed 1.5\n", "roi_x 2147483648\n", "log_delta x\n"}) {
    CHECK(!load_ground_file(file_of(text).c_str(), &g, &log_delta, &err), "%s accepted", text);
    CHECK(!memcmp(&g, &g0, sizeof g) && log_delta == 9.f, "%s stored something", text);
  }
  sn_elevation_params e = default_elevation_params(), e0 = e;
  bool feed = true;
  CHECK(!load_elevation_file(file_of("mw 1.5\n").c_str(), &e, &frame, &feed, &err) && !memcmp(&e, &e0, sizeof e) && feed, "elevation mw 1.5");
  CHECK(!load_elevation_file(file_of("feed_inflate 2\n").c_str(), &e, &frame, &feed, &err) && err == "feed_inflate must be 0 or 1" && feed, "feed_inflate 2: %s", err.c_str());
  CHECK(!load_elevation_file(file_of("feed_inflate -1\n").c_str(), &e, &frame, &feed, &err) && err == "feed_inflate must be 0 or 1", "feed_inflate -1: %s", err.c_str());
  CHECK(!load_elevation_file(file_of("feed_inflate 1.5\n").c_str(), &e, &frame, &feed, &err) && err == "line 1: wrong values for feed_inflate", "feed_inflate 1.5: %s", err.c_str());
  CHECK(load_elevation_file(file_of("feed_inflate 0\n").c_str(), &e, &frame, &feed, &err) && !feed, "feed_inflate 0");
  CHECK(load_elevation_file(file_of("feed_inflate 1\n").c_str(), &e, &frame, &feed, &err) && feed, "feed_inflate 1");
  sn_rollout_params r = default_rollout_params(), r0 = r;
  std::vector<float> fp;
  double acc[3] = {7.0, 8.0, 9.0};
  bool has_acc = false;
  for (const char* text : {"acc 1 2\n", "acc 1 2 3 4\n", "acc 1 2 x\n", "pose 1 2\n", "pose 1 2 3 4\n", "pose 1 x 3\n", "point 1\n", "point 1 2 3\n", "point 1 x\n",
                           "nv 3e10\n", "v_max x\n"}) {
    CHECK(!load_rollout_file(file_of(text).c_str(), &r, &fp, acc, &has_acc, &err), "%s accepted", text);
    CHECK(!memcmp(&r, &r0, sizeof r) && fp.empty() && !has_acc && acc[0] == 7.0 && acc[1] == 8.0 && acc[2] == 9.0, "%s stored something", text);
  }
  CHECK(load_rollout_file(file_of("point 1 2\npoint 3 4 # again\npose 1 2 3\nacc 0.5 nan 3\npoint -1 -2\n").c_str(), &r, &fp, acc, &has_acc, &err), "rollout: %s", err.c_str());
  CHECK(fp == std::vector<float>({1.f, 2.f, 3.f, 4.f, -1.f, -2.f}) && has_acc && acc[0] == 0.5 && acc[1] != acc[1] && acc[2] == 3.0, "rollout's side outputs");
  sn_nav_params v = default_plan_params(), v0 = v;
  for (const char* text : {"goal 1\n", "goal 1 2 3\n", "goal 1.5 2\n", "start 1 3e10\n", "start x 1\n", "max_rounds 2147483648\n"}) {
    CHECK(!load_plan_file(file_of(text).c_str(), &v, &err) && err.find("line 1: wrong values for ") == 0, "%s: %s", text, err.c_str());
    CHECK(!memcmp(&v, &v0, sizeof v), "%s stored something", text);
  }
  CHECK(load_plan_file(file_of("goal 1 2\nstart 3 4\nmax_rounds 2000000000\n").c_str(), &v, &err) && v.max_rounds == 2000000000, "plan: %s", err.c_str());
  sn_stereo_calib c{};
  CHECK(!load_calib_file(file_of(file_text(0, 0, "size 640.5 480\n")).c_str(), &c, &err) && err == "size is not two integers", "size 640.5: %s", err.c_str());
  CHECK(!load_calib_file(file_of(file_text(0, 0, "size 640 3e10\n")).c_str(), &c, &err) && err == "size is not two integers", "size 3e10: %s", err.c_str());
  CHECK(!load_calib_file(file_of(file_text(0, 0, "size nan 480\n")).c_str(), &c, &err) && err == "size is not two integers", "size nan: %s", err.c_str());
  CHECK(load_calib_file(file_of(file_text(0, 0, "size 640 480\n")).c_str(), &c, &err) && c.src_w == 640 && c.src_h == 480 && c.left.fx == 1.0 && c.pcy == 1.0, "calib: %s", err.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "dump") && kind_of(argv[2]) >= 0) {
    for (int i = 3; i < argc; ++i) {
      if (argc > 4) printf("== %s\n", argv[i]);
      fputs(dump(kind_of(argv[2]), argv[i]).c_str(), stdout);
    }
    return 0;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: param_file_check [dump calib|obstacle|ground|costmap|elevation|inflate|plan|rollout FILE...]\n");
    return 2;
  }
  char dir[] = "/tmp/param_file_check.XXXXXX";
  if (!mkdtemp(dir)) return perror("mkdtemp"), 2;
  g_dir = dir;
  for (int kind = 0; kind < 8; ++kind) cases_of(kind);
  refused_values_store_nothing();
  for (int i = 0; i < g_files; ++i) unlink((g_dir + "/f" + std::to_string(i)).c_str());
  rmdir(dir);
  if (failures) return fprintf(stderr, "param_file_check: %d failures\n", failures), 1;
  puts("param_file_check: ok");
  return 0;
}
