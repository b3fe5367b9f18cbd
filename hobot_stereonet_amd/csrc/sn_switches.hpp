// sn_switches.hpp — every SN_* environment switch the library reads: ONE table (struct Switches), one function that fills
// it from the environment (read_switches) and one accessor (switches).  No other file under csrc/ calls getenv("SN_...")
// (csrc/compat and its STEREONET_* / SN_LOG_LEVEL variables are a separate program).  INTEGRATION.md §3 documents the
// same list; tests/test_switches.py keeps the two in step.
#pragma once

#include <cctype>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/stereonet_hip.h"

#ifndef SN_DIAGNOSTICS
#define SN_DIAGNOSTICS 0      // 1: the precision-ablation switches of scripts/lowres_ablation.py (never in the shipping library)
#endif

namespace sn {

constexpr int kSwitchUnset = INT_MIN;      // an integer switch that is not in the environment

// layer numbering of SN_ABLATE_W / SN_ABLATE_X: down1..down3, f0..f12 (the thirteen 3x3 feature convs), agg0..agg3
enum { kAblDown = 0, kAblFeat = 3, kAblAgg = 16, kAblCount = 20 };

// One field per switch:  variable | default | scope | meaning.
//   scope process: latched for the life of the process, at the first use of any switch (the first sn_create at the latest)
//   scope create:  read again by every sn_create / sn_mgpu_create (and by a parity hook that uploads weights), so one
//                  process can hold engines that differ in it; the value lands in the handle
// On/off switches: unset or any non-zero integer = on, 0 = off.  "presence": set to anything = on.
struct Switches {
  bool down01 = true;          // SN_DOWN01 | 1 | process | 0: k_down0_f16 + the 5x5 stride-2 kernel instead of the folded 13x13 stride-4 conv
  bool agg_dma = true;         // SN_AGG_DMA | 1 | process | 0: aggregation layers on plain split-slot volumes (k_conv_x3s), not the zero-bordered ones
  bool feat_dma = true;        // SN_FEAT_DMA | 1 | process | 0: the same for the 3x3 feature layers
  bool down_dma = true;        // SN_DOWN_DMA | 1 | process | 0: the same for down-convs 1..3
  bool head_fold = true;       // SN_HEAD_FOLD | 1 | process | 0: the last aggregation layer writes its volume, k_head_softargmin contracts it
  int f32_grid = 0;            // SN_F32_GRID | 0 | process | n > 0: workgroups per fp32 tower launch (probe; 0 = one per CU)
  bool f32_tower = true;       // SN_F32_TOWER | 1 | process | 0: SN_PREC_FP32 keeps the generic kernel for the tower layers too
  int stream_wgs = 0;          // SN_STREAM_WGS | 0 | process | n > 0: workgroups of a streamed fp16 block launch (experiment; 0 = one per CU)
  int stream_dil = 8;          // SN_STREAM_DIL | 8 | process | largest dilation that runs through the streaming fp16 block kernel
  int fuse = 4;                // SN_FUSE | 4 | process | fp16 tower blocks: 4 = row-streaming fused kernel, 0 = two launches per block
  bool x3_stream = true;       // SN_X3_STREAM | 1 | process | 0: two k_ref_conv_f16x3 launches per split block instead of the streamed one
  int x3_nwr = 4;              // SN_X3_NWR | 4 | process | waves per role of the streamed split block: 4 = two per SIMD, 2 = one
  int first_piece = 0;         // SN_FIRST_PIECE | 0 | process | n > 0: pairs in the first low-resolution piece of a pipelined forward (experiment)
  bool head_mfma32 = true;     // SN_HEAD_MFMA32 | 1 | process | 0: SN_PREC_FP32 head as the per-pixel k_head_final
  bool rev = true;             // SN_REV | 1 | process | 0: every tower launch walks its tiles in the same direction
  bool async_share = true;     // SN_ASYNC_SHARE | 1 | process | 0: an async request keeps every CU while others are in flight

  bool w_round_sum_preserving = true;      // SN_W_ROUND | sum | create | rne: round-to-nearest fp16 tower weights instead of the sum-preserving rounding
  int precision = SN_PREC_AUTO;            // SN_PRECISION | auto | create | f16, f16x3, fp32, auto: what SN_PREC_DEFAULT means
  int tower_streams = kSwitchUnset;        // SN_TOWER_STREAMS | unset | create | tower streams (unset: 2 in SN_PREC_FP32, else 1)
  int stream_priority = kSwitchUnset;      // SN_STREAM_PRIORITY | unset | create | 1 / 0: pipeline streams at the highest priority or not, whatever the caller asked
  bool no_overlap = false;                 // SN_NO_OVERLAP | unset | create | presence: single-stream execution
  bool no_graph = false;                   // SN_NO_GRAPH | unset | create | presence: no hipGraph replay in the async slots
  bool tail_fuse = true;                   // SN_TAIL_FUSE | 1 | create | 0: last streamed block + k_head_final_f16 instead of the tail form
  bool obstacle_rle = true;                // SN_OBSTACLE_RLE | 1 | create | 0: sn_obstacles_from_raw sends one set of atomics per point instead of one per run of a lane
  int inflate_waves = 0;                   // SN_INFLATE_WAVES | 0 | create | 4 or 16: waves per workgroup of k_inflate whatever the call's size (0: 16 while all its workgroups are resident at once, else 4)
  int mgpu_gather = 0;                     // SN_MGPU_GATHER | unset | create | peer (1) or rccl (2): forces the exchange of sn_mgpu_*
  bool mgpu_allow_dup = false;             // SN_MGPU_ALLOW_DUP | 0 | create | 1: several shards may name one device (tests)
  // Diagnostic build only (-DSN_DIAGNOSTICS=1); the shipping library never reads them and both masks stay 0.  Any
  // SN_ABLATE_X at the time the process switches are latched also forces the plain layouts (agg_dma = feat_dma = down_dma = false).
  unsigned ablate_w = 0;       // SN_ABLATE_W | unset | create | layers whose weights lose their lo fragments
  unsigned ablate_x = 0;       // SN_ABLATE_X | unset | create | layers whose input tensor gets its lo slots zeroed
};

namespace switch_parse {
inline bool on_unless_zero(const char* name) {
  const char* e = getenv(name);
  return !(e != nullptr && atoi(e) == 0);
}
inline bool present(const char* name) { return getenv(name) != nullptr; }
inline int int_or(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline bool equals(const char* name, const char* value) {
  const char* e = getenv(name);
  return e && strcmp(e, value) == 0;
}

// <layers>: comma-separated names out of down1..down3, f0..f12, agg0..agg3, or "all"
#if !SN_DIAGNOSTICS
inline unsigned ablate_mask(const char*) { return 0u; }
#else
inline unsigned ablate_mask(const char* var) {
  const char* e = getenv(var);
  if (!e || !*e) return 0u;
  if (!strcmp(e, "all")) return (1u << kAblCount) - 1u;
  unsigned m = 0;
  std::string str(e);
  size_t pos = 0;
  while (pos <= str.size()) {
    size_t c = str.find(',', pos);
    if (c == std::string::npos) c = str.size();
    const std::string t = str.substr(pos, c - pos);
    int idx = -1;
    if (t.rfind("down", 0) == 0 && t.size() == 5 && t[4] >= '1' && t[4] <= '3') idx = kAblDown + (t[4] - '1');
    else if (t.rfind("agg", 0) == 0 && t.size() == 4 && t[3] >= '0' && t[3] <= '3') idx = kAblAgg + (t[3] - '0');
    else if (t.size() >= 2 && t[0] == 'f' && atoi(t.c_str() + 1) >= 0 && atoi(t.c_str() + 1) <= 12 && isdigit((unsigned char)t[1])) idx = kAblFeat + atoi(t.c_str() + 1);
    if (idx >= 0) m |= 1u << idx;
    pos = c + 1;
  }
  return m;
}
#endif
}  // namespace switch_parse

// Fills the fields of one scope from the environment.
inline void read_switches(Switches* s, bool process_scope) {
  using namespace switch_parse;
  if (process_scope) {
    const bool plain = ablate_mask("SN_ABLATE_X") != 0;
    s->down01 = on_unless_zero("SN_DOWN01");
    s->agg_dma = on_unless_zero("SN_AGG_DMA") && !plain;
    s->feat_dma = on_unless_zero("SN_FEAT_DMA") && !plain;
    s->down_dma = on_unless_zero("SN_DOWN_DMA") && !plain;
    s->head_fold = on_unless_zero("SN_HEAD_FOLD");
    s->f32_grid = int_or("SN_F32_GRID", 0);
    s->f32_tower = on_unless_zero("SN_F32_TOWER");
    s->stream_wgs = int_or("SN_STREAM_WGS", 0);
    s->stream_dil = int_or("SN_STREAM_DIL", 8);
    s->fuse = int_or("SN_FUSE", 4);
    s->x3_stream = on_unless_zero("SN_X3_STREAM");
    s->x3_nwr = int_or("SN_X3_NWR", 4);
    s->first_piece = int_or("SN_FIRST_PIECE", 0);
    s->head_mfma32 = on_unless_zero("SN_HEAD_MFMA32");
    s->rev = on_unless_zero("SN_REV");
    s->async_share = on_unless_zero("SN_ASYNC_SHARE");
    return;
  }
  s->w_round_sum_preserving = !equals("SN_W_ROUND", "rne");
  s->precision = equals("SN_PRECISION", "f16") ? SN_PREC_F16 : equals("SN_PRECISION", "f16x3") ? SN_PREC_F16X3
                 : equals("SN_PRECISION", "fp32") ? SN_PREC_FP32 : SN_PREC_AUTO;
  s->tower_streams = int_or("SN_TOWER_STREAMS", kSwitchUnset);
  s->stream_priority = equals("SN_STREAM_PRIORITY", "") ? kSwitchUnset : int_or("SN_STREAM_PRIORITY", kSwitchUnset);      // empty = unset
  s->no_overlap = present("SN_NO_OVERLAP");
  s->no_graph = present("SN_NO_GRAPH");
  s->tail_fuse = on_unless_zero("SN_TAIL_FUSE");
  s->obstacle_rle = on_unless_zero("SN_OBSTACLE_RLE");
  s->inflate_waves = int_or("SN_INFLATE_WAVES", 0);
  s->mgpu_gather = equals("SN_MGPU_GATHER", "peer") ? 1 : equals("SN_MGPU_GATHER", "rccl") ? 2 : 0;
  s->mgpu_allow_dup = int_or("SN_MGPU_ALLOW_DUP", 0) == 1;
  s->ablate_w = ablate_mask("SN_ABLATE_W");
  s->ablate_x = ablate_mask("SN_ABLATE_X");
}

// switches(): the process-scope fields, latched at the first call; its create-scope fields hold their defaults.
// switches_at_create() (sn_create, sn_mgpu_create, parity hooks that upload tower weights): a copy of it whose
// create-scope fields have just been read from the environment.
inline const Switches& switches() {
  static const Switches latched = [] {
    Switches s;
    read_switches(&s, true);
    return s;
  }();
  return latched;
}
inline Switches switches_at_create() {
  Switches s = switches();
  read_switches(&s, false);
  return s;
}

}  // namespace sn
