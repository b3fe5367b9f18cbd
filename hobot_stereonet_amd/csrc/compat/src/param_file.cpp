// param_file.cpp — all line handling of the `key value...` files: the comment strip, the split, the repeated-key test, the
// number test and the error text
#include "param_file.h"

#include <cstdlib>
#include <fstream>
#include <sstream>

namespace hobot {
namespace stereonet {

bool read_param_file(const char* path, const std::vector<ParamKey>& keys, bool all_required, std::string* err) {
  std::ifstream in(path);
  if (!in.good()) {
    *err = "cannot be opened";
    return false;
  }
  std::vector<bool> seen(keys.size(), false);
  std::string text;
  for (int no = 1; std::getline(in, text); ++no) {
    std::istringstream words(text.substr(0, text.find('#')));
    std::string name, w;
    if (!(words >> name)) continue;
    std::vector<std::string> vals;
    while (words >> w) vals.push_back(w);
    size_t k = 0;
    while (k < keys.size() && name != keys[k].name) ++k;
    const std::string at = "line " + std::to_string(no) + ": ";
    if (k == keys.size()) {      // a key seen before is known: `twice` can only come first
      *err = at + "unknown key " + name;
      return false;
    }
    const ParamKey& key = keys[k];
    if (seen[k] && key.kind != ParamKind::kAppend) {
      *err = at + name + " twice";
      return false;
    }
    seen[k] = true;
    bool ok = (int)vals.size() == key.count;
    std::vector<double> num(vals.size(), 0.0);
    for (size_t i = 0; ok && i < vals.size() && key.kind != ParamKind::kWord; ++i) {
      char* end = nullptr;
      num[i] = strtod(vals[i].c_str(), &end);
      ok = end != vals[i].c_str() && !*end;
      if (key.kind == ParamKind::kInt) ok = ok && is_int32(num[i]);
      if (key.kind == ParamKind::kUint32) ok = ok && integral_in(num[i], 0.0, 4294967295.0);
    }
    if (!ok) {
      *err = at + "wrong values for " + name;
      return false;
    }
    if (key.present) *key.present = true;
    for (int i = 0; key.dst && i < key.count; ++i) switch (key.kind) {
        case ParamKind::kFloat: static_cast<float*>(key.dst)[i] = (float)num[i]; break;
        case ParamKind::kDouble: static_cast<double*>(key.dst)[i] = num[i]; break;
        case ParamKind::kInt: static_cast<int*>(key.dst)[i] = (int)num[i]; break;
        case ParamKind::kUint32: static_cast<uint32_t*>(key.dst)[i] = (uint32_t)num[i]; break;
        case ParamKind::kWord: *static_cast<std::string*>(key.dst) = vals[i]; break;
        case ParamKind::kAppend: static_cast<std::vector<float>*>(key.dst)->push_back((float)num[i]); break;
      }
  }
  for (size_t k = 0; all_required && k < keys.size(); ++k)
    if (!seen[k]) {
      *err = std::string("has no `") + keys[k].name + "` line";
      return false;
    }
  return true;
}

}  // namespace stereonet
}  // namespace hobot
