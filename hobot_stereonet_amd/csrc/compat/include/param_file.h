// param_file.h — the one reader of the `key value...` text files that the node's stages and the tools share (the Python
// twin is hobot_stereonet_amd/paramfile.py).  One key a line, `#` starts a comment, a key at most once; a key that is missing
// keeps what its destination held.  Host only: no engine symbol.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace hobot {
namespace stereonet {

// how a key's values are tested and stored.  kInt / kUint32: a number in the type's range that is integral, the range tested
// before the cast.  kWord: any one word.  kAppend: floats pushed onto a vector, and the one kind whose key may repeat
enum class ParamKind { kFloat, kDouble, kInt, kUint32, kWord, kAppend };

struct ParamKey {
  const char* name;
  ParamKind kind;
  int count;                 // values on the line
  void* dst;                 // count of them, of the kind's type; nullptr: read past (the values are still tested)
  bool* present = nullptr;   // set once the key was accepted
  ParamKey(const char* n, float* v, int c = 1) : name(n), kind(ParamKind::kFloat), count(c), dst(v) {}
  ParamKey(const char* n, double* v, int c = 1, bool* seen = nullptr) : name(n), kind(ParamKind::kDouble), count(c), dst(v), present(seen) {}
  ParamKey(const char* n, int* v) : name(n), kind(ParamKind::kInt), count(1), dst(v) {}
  ParamKey(const char* n, uint32_t* v) : name(n), kind(ParamKind::kUint32), count(1), dst(v) {}
  ParamKey(const char* n, std::string* v) : name(n), kind(ParamKind::kWord), count(1), dst(v) {}
  ParamKey(const char* n, std::vector<float>* v, int c) : name(n), kind(ParamKind::kAppend), count(c), dst(v) {}
  ParamKey(const char* n, ParamKind k, int c) : name(n), kind(k), count(c), dst(nullptr) {}      // read past
};

// whether d is an integer of [lo, hi]; false for NaN
inline bool integral_in(double d, double lo, double hi) { return d >= lo && d <= hi && d == (double)(int64_t)d; }
inline bool is_int32(double d) { return integral_in(d, -2147483648.0, 2147483647.0); }

// false: *err is `cannot be opened`, `line N: KEY twice`, `line N: unknown key KEY`, `line N: wrong values for KEY` (tested in
// this order) or, with all_required, "has no `KEY` line" for the first key of the table that the file lacks.  A line that is
// refused stores nothing.
bool read_param_file(const char* path, const std::vector<ParamKey>& keys, bool all_required, std::string* err);

}  // namespace stereonet
}  // namespace hobot
