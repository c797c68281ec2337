// rplgpu_frontier_rules.cpp — the rules of E29, a map's frontiers found, grouped and the next goal picked
// (include/rplgpu_msg.h), in plain C++: the default, the check, the scratch size and the host twin — a flood fill over
// the frontier cells in ascending cell index ("the definition a reader can run").  No handle, no stream, no HIP
// header; built like rplgpu_nav_rules.cpp.  The doors that call these are in rplgpu_frontier_stages.hip;
// tools/dev/plan_rules_asan.cpp drives this file under the host sanitizers.
#include <cstring>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_frontier.hpp"

namespace {

struct Comp {
  uint32_t label, n;
  uint64_t sx, sy, key;
};

void put_row(uint32_t *row, const Comp &c) {
  row[0] = c.label;
  row[1] = c.n;
  row[2] = (uint32_t)c.sx;
  row[3] = (uint32_t)(c.sx >> 32);
  row[4] = (uint32_t)c.sy;
  row[5] = (uint32_t)(c.sy >> 32);
  row[6] = (uint32_t)(c.key >> 32);
  row[7] = (uint32_t)c.key;
}

}  // namespace

extern "C" {

void rplgpu_default_frontiers(rplgpu_frontiers_t *f) {
  if (!f) return;
  f->width = 1024;
  f->height = 1024;
  f->lethal = 99;
  f->min_size = 8;
  f->dist_weight = 1;
  f->size_weight = 0;
}

int32_t rplgpu_frontiers_check(const rplgpu_frontiers_t *f) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (f->width == 0 || f->width > RPLGPU_MAX_OCC_DIM || f->height == 0 || f->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (f->lethal == 0 || f->lethal > 100u || f->min_size == 0 || f->dist_weight > 65535u || f->size_weight > 65535u)
    return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_frontiers_scratch_words(const rplgpu_frontiers_t *f, uint32_t G, uint32_t comp_cap) {
  rpl::FrLayout l;
  if (rplgpu_frontiers_check(f) != RPLGPU_OK || !rpl::frontier_layout(f->width, f->height, G, comp_cap, &l)) return 0;
  return l.total * G;
}

int32_t rplgpu_frontiers_host(const rplgpu_frontiers_t *f, const int8_t *grid, const uint32_t *potential,
                              uint32_t comp_cap, uint32_t *labels_out, uint32_t *rows, uint32_t row_cap,
                              uint32_t *goal_out, uint32_t *n_goal_out, uint32_t result[16]) {
  if (rplgpu_frontiers_check(f) != RPLGPU_OK || !grid || !result || comp_cap == 0 ||
      comp_cap > RPLGPU_FRONTIER_MAX_COMPS || (row_cap != 0 && !rows) || (!goal_out) != (!n_goal_out))
    return RPLGPU_ERR_INVALID_ARG;
  const int w = (int)f->width, h = (int)f->height;
  const size_t cells = (size_t)w * h;
  const auto unknown = [&](int x, int y) { return x >= 0 && y >= 0 && x < w && y < h && grid[(size_t)y * w + x] < 0; };
  std::vector<uint32_t> label(cells, RPLGPU_FRONTIER_NO_LABEL);
  std::vector<uint8_t> frontier(cells, 0);
  uint32_t F = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t c = (size_t)y * w + x;
      const int8_t v = grid[c];
      if (v < 0 || (uint32_t)v >= f->lethal || (potential && potential[c] == RPLGPU_NAV_UNREACHED)) continue;
      if (unknown(x + 1, y) || unknown(x - 1, y) || unknown(x, y + 1) || unknown(x, y - 1)) {
        frontier[c] = 1;
        ++F;
      }
    }
  // the fill: seeds in ascending cell index, so a component's seed is its label
  std::vector<Comp> comps;
  std::vector<uint32_t> stack;
  for (size_t seed = 0; seed < cells; ++seed) {
    if (!frontier[seed] || label[seed] != RPLGPU_FRONTIER_NO_LABEL) continue;
    Comp c{(uint32_t)seed, 0, 0, 0, ~0ull};
    label[seed] = (uint32_t)seed;
    stack.push_back((uint32_t)seed);
    while (!stack.empty()) {
      const uint32_t at = stack.back();
      stack.pop_back();
      const int x = (int)(at % (uint32_t)w), y = (int)(at / (uint32_t)w);
      ++c.n;
      c.sx += (uint64_t)x;
      c.sy += (uint64_t)y;
      const uint64_t key = ((uint64_t)(potential ? potential[at] : 0u) << 32) | at;
      if (key < c.key) c.key = key;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int nx = x + dx, ny = y + dy;
          if (nx < 0 || ny < 0 || nx >= w || ny >= h) continue;
          const size_t q = (size_t)ny * w + nx;
          if (!frontier[q] || label[q] != RPLGPU_FRONTIER_NO_LABEL) continue;
          label[q] = (uint32_t)seed;
          stack.push_back((uint32_t)q);
        }
    }
    comps.push_back(c);
  }
  const uint32_t N = (uint32_t)comps.size();
  uint32_t words[16] = {0, F, N, 0, 0, RPLGPU_FRONTIER_NO_LABEL, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const Comp *best = nullptr;
  if (N > comp_cap) {
    words[0] |= RPLGPU_FRONTIER_BOUND;
  } else {
    int64_t best_cost = 0;
    for (const Comp &c : comps) {  // (ascending label)
      if (c.n > words[13]) words[13] = c.n;
      if (c.n < f->min_size) {
        words[4] += c.n;
        continue;
      }
      if (words[3] < row_cap) {
        put_row(rows + 8u * (size_t)words[3], c);
        ++words[14];
      }
      ++words[3];
      const int64_t cost = (int64_t)f->dist_weight * (int64_t)(c.key >> 32) - (int64_t)f->size_weight * (int64_t)c.n;
      if (!best || cost < best_cost) {
        best = &c;
        best_cost = cost;
      }
    }
  }
  if (F == 0) words[0] |= RPLGPU_FRONTIER_NONE;
  if (best) {
    uint32_t row[8];
    put_row(row, *best);
    words[5] = row[0];
    words[6] = row[1];
    words[7] = row[6];
    words[8] = row[7];
    std::memcpy(words + 9, row + 2, 16);
  } else {
    words[0] |= RPLGPU_FRONTIER_NO_KEPT;
  }
  if (labels_out) std::memcpy(labels_out, label.data(), 4u * cells);
  if (goal_out) {
    if (best) *goal_out = (uint32_t)best->key;
    *n_goal_out = best ? 1u : 0u;
  }
  std::memcpy(result, words, sizeof(words));
  return RPLGPU_OK;
}

}  // extern "C"
