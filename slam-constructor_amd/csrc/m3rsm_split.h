// m3rsm_split.h -- how a translation rectangle of the multi-resolution matcher is refined, stated once for the host
// engine (m3rsm_engine.cpp) and the expand kernel (m3rsm.hip).
//
// What it restates (paths relative to the reference root):
//   M3RSMEngine::next_best_match / branch          src/core/scan_matchers/m3rsm_engine.h:318-357
//   BruteForceMultiResolutionScanMatcher           src/core/scan_matchers/bf_multi_res_scan_matcher.h:45-64 (five points)
//   LightWeightRectangle::center / split_*         src/core/geometry_primitives.h:188-244
//   less                                           src/core/math_utils.h:22-25
//
// Plain FP64 in the reference's operation order; compile with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define SLAMHIP_M3RSM_FN __host__ __device__ static inline
#else
#define SLAMHIP_M3RSM_FN static inline
#endif

namespace slamhip {
namespace m3rsm {

constexpr int kMaxChildren = 5;  // child slots per node: four quarters at most, or the five crucial points
constexpr int kMaxDepth = 3;     // generations one expand launch scores

struct Rect {
  double bot, top, left, right;
};

// less(a, b) of math_utils.h: a < b + DBL_EPSILON
SLAMHIP_M3RSM_FN bool less(double a, double b) { return a < b + 2.220446049250313e-16; }

// a rectangle the reference could hold: finite, bot <= top, left <= right
SLAMHIP_M3RSM_FN bool is_rect(const Rect &r) {
  const double v = r.top - r.bot, h = r.right - r.left;
  return v >= 0.0 && h >= 0.0 && v < __builtin_inf() && h < __builtin_inf();
}

// Match::is_finest(): the rectangle is a point
SLAMHIP_M3RSM_FN bool is_finest(const Rect &r) { return (r.right - r.left) + (r.top - r.bot) <= 0.0; }

// slots of one parent to depth d, breadth first: 5 + 25 + ... + 5^d
SLAMHIP_M3RSM_FN int slots_of(int depth) { return depth == 1 ? 5 : depth == 2 ? 30 : 155; }

// Child c (0 .. 4) of `r` under the translation step, in the reference's order; false where `r` has fewer children.
//   both sides branch (less(step, side)): split4_evenly's four; one side: split_horz's / split_vert's two; neither and
//   not a point: the corners (left, bot), (left, top), (right, bot), (right, top) and the centre as point rectangles
//   {y, y, x, x}; a point, or something that is no rectangle, has none.
// (One child at a time, chosen by selects: the kernel keeps no array of rectangles, hence no scratch memory.)
SLAMHIP_M3RSM_FN bool child_at(const Rect &r, double step, int c, Rect *out) {
  if (!is_rect(r) || c < 0) return false;
  const double hside = r.right - r.left, vside = r.top - r.bot;
  const bool hb = less(step, hside), vb = less(step, vside);
  const double cx = r.left + hside / 2, cy = r.bot + vside / 2;
  if (hb && vb) {  // left-bot, left-top, right-bot, right-top
    if (c >= 4) return false;
    const bool up = (c & 1) != 0, east = c >= 2;
    *out = Rect{up ? cy : r.bot, up ? r.top : cy, east ? cx : r.left, east ? r.right : cx};
    return true;
  }
  if (hb) {
    if (c >= 2) return false;
    *out = Rect{r.bot, r.top, c ? cx : r.left, c ? r.right : cx};
    return true;
  }
  if (vb) {
    if (c >= 2) return false;
    *out = Rect{c ? cy : r.bot, c ? r.top : cy, r.left, r.right};
    return true;
  }
  if (is_finest(r) || c >= kMaxChildren) return false;
  const double y = c == 4 ? cy : ((c & 1) ? r.top : r.bot), x = c == 4 ? cx : (c >= 2 ? r.right : r.left);
  *out = Rect{y, y, x, x};
  return true;
}

// all children of `r`; returns how many (0, 2, 4 or 5)
SLAMHIP_M3RSM_FN int children(const Rect &r, double step, Rect out[kMaxChildren]) {
  int n = 0;
  while (n < kMaxChildren && child_at(r, step, n, &out[n])) ++n;
  return n;
}

// The node of slot `s` (0 .. slots_of(depth) - 1) under `parent`: generation g holds 5^g slots, slot j of it being child
// j % 5 of slot j / 5 of the generation before.  False where the path meets a node with fewer children.
SLAMHIP_M3RSM_FN bool slot_node(const Rect &parent, double step, int s, Rect *node) {
  int gen = 1, j = s, width = kMaxChildren;
  while (j >= width) {
    j -= width;
    width *= kMaxChildren;
    ++gen;
  }
  Rect r = parent;
  for (int g = gen; g >= 1; --g) {
    width /= kMaxChildren;  // 5^(g - 1): slots of this generation under one child of the node at hand
    const int c = j / width;
    j -= c * width;
    Rect kid;
    if (!child_at(r, step, c, &kid)) return false;
    r = kid;
  }
  *node = r;
  return true;
}

}  // namespace m3rsm
}  // namespace slamhip
