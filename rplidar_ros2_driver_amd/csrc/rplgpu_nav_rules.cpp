// rplgpu_nav_rules.cpp — the rules of E26, the cost-to-goal field over a costmap and the paths down it
// (include/rplgpu_msg.h), in plain C++: the default, the check, the default rounds, the scratch size and the host
// twins — a binary-heap Dijkstra from the goals ("the definition a reader can run") and the downhill walk.  No
// handle, no stream, no HIP header; built like rplgpu_pose_rules.cpp.  The doors that call these are in
// rplgpu_nav_stages.hip; tools/dev/plan_rules_asan.cpp drives this file under the host sanitizers.
#include <algorithm>
#include <cstring>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "rplgpu.h"
#include "rplgpu_msg.h"
#include "rpl_rules.hpp"

namespace {

const int kDx[8] = {1, -1, 0, 0, 1, -1, 1, -1};
const int kDy[8] = {0, 0, 1, -1, 1, 1, -1, -1};

struct Grid {
  const rplgpu_nav_field_t *f;
  const int8_t *bytes;
  int w, h;
  bool inside(int x, int y) const { return x >= 0 && y >= 0 && x < w && y < h; }
  uint32_t weight(int x, int y) const { return rpl::nav_byte_weight(*f, bytes[(size_t)y * w + x]); }
  // the step `dir` from (x, y): the neighbour inside the grid, (x, y) passable, no corner cut
  bool allowed(int x, int y, int dir) const {
    const int nx = x + kDx[dir], ny = y + kDy[dir];
    if (!inside(nx, ny) || weight(x, y) == 0) return false;
    return dir < 4 || (weight(nx, y) != 0 && weight(x, ny) != 0);
  }
};

}  // namespace

extern "C" {

uint32_t rplgpu_nav_field_default_rounds(uint32_t width, uint32_t height) {
  if (width == 0 || width > RPLGPU_MAX_OCC_DIM || height == 0 || height > RPLGPU_MAX_OCC_DIM) return 0;
  uint32_t tiles_x, tiles_y;
  (void)rpl::nav_tiles(width, height, 1, &tiles_x, &tiles_y);
  return 2u * (tiles_x + tiles_y) + 2u;
}

void rplgpu_default_nav_field(rplgpu_nav_field_t *f) {
  if (!f) return;
  f->width = 1024;
  f->height = 1024;
  f->lethal = 99;
  f->neutral = 50;
  f->factor = 2;
  f->unknown_cost = 0;
  f->cap = RPLGPU_NAV_MAX_CAP;
  f->rounds = rplgpu_nav_field_default_rounds(f->width, f->height);
}

int32_t rplgpu_nav_field_check(const rplgpu_nav_field_t *f) {
  if (!f) return RPLGPU_ERR_INVALID_ARG;
  if (f->width == 0 || f->width > RPLGPU_MAX_OCC_DIM || f->height == 0 || f->height > RPLGPU_MAX_OCC_DIM)
    return RPLGPU_ERR_INVALID_ARG;
  if (f->lethal == 0 || f->lethal > 100u || f->neutral == 0 || f->neutral > 255u || f->factor > 16u)
    return RPLGPU_ERR_INVALID_ARG;
  if (f->unknown_cost > RPLGPU_NAV_MAX_COST || f->cap > RPLGPU_NAV_MAX_CAP) return RPLGPU_ERR_INVALID_ARG;
  if (f->rounds == 0 || f->rounds > RPLGPU_NAV_MAX_ROUNDS) return RPLGPU_ERR_INVALID_ARG;
  if (f->neutral + f->factor * (f->lethal - 1u) > RPLGPU_NAV_MAX_COST) return RPLGPU_ERR_INVALID_ARG;
  return RPLGPU_OK;
}

uint64_t rplgpu_nav_field_scratch_words(const rplgpu_nav_field_t *f, uint32_t G) {
  if (rplgpu_nav_field_check(f) != RPLGPU_OK || G == 0) return 0;
  uint32_t tiles_x, tiles_y;
  if (!rpl::nav_tiles(f->width, f->height, G, &tiles_x, &tiles_y)) return 0;
  return 2ull * tiles_x * tiles_y * G;
}

int32_t rplgpu_nav_field_host(const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *goals,
                              uint32_t n_goals, uint32_t *potential, uint32_t result[8]) {
  if (rplgpu_nav_field_check(f) != RPLGPU_OK || !grid || !potential || (n_goals != 0 && !goals))
    return RPLGPU_ERR_INVALID_ARG;
  const Grid g{f, grid, (int)f->width, (int)f->height};
  const size_t cells = (size_t)f->width * f->height;
  std::fill(potential, potential + cells, RPLGPU_NAV_UNREACHED);
  typedef std::pair<uint32_t, uint32_t> Entry;  // (D, cell)
  std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
  uint32_t taken = 0, ignored = 0;
  for (uint32_t i = 0; i < n_goals; ++i) {
    if (i >= RPLGPU_NAV_MAX_GOALS || goals[i] >= cells) {
      ++ignored;
      continue;
    }
    ++taken;
    if (potential[goals[i]] != 0) {
      potential[goals[i]] = 0;
      heap.push(Entry(0u, goals[i]));
    }
  }
  while (!heap.empty()) {
    const Entry e = heap.top();
    heap.pop();
    if (potential[e.second] != e.first) continue;  // (an entry a later, smaller one replaced)
    const int nx = (int)(e.second % f->width), ny = (int)(e.second / f->width);
    // every cell c with an allowed step c -> n
    for (int dir = 0; dir < 8; ++dir) {
      const int cx = nx - kDx[dir], cy = ny - kDy[dir];
      if (!g.inside(cx, cy) || !g.allowed(cx, cy, dir)) continue;
      const uint64_t cand = (uint64_t)e.first + (uint64_t)(dir < 4 ? 5u : 7u) * g.weight(cx, cy);
      const size_t c = (size_t)cy * f->width + (size_t)cx;
      if (cand <= f->cap && cand < potential[c]) {
        potential[c] = (uint32_t)cand;
        heap.push(Entry((uint32_t)cand, (uint32_t)c));
      }
    }
  }
  if (result) {
    uint32_t reached = 0, greatest = 0;
    for (size_t c = 0; c < cells; ++c)
      if (potential[c] != RPLGPU_NAV_UNREACHED) {
        ++reached;
        greatest = std::max(greatest, potential[c]);
      }
    const uint32_t words[8] = {0, 0, taken, ignored, reached, greatest, 0, 0};
    std::memcpy(result, words, sizeof(words));
  }
  return RPLGPU_OK;
}

int32_t rplgpu_nav_path_host(const rplgpu_nav_field_t *f, const int8_t *grid, const uint32_t *potential,
                             uint32_t start, uint32_t *path, uint32_t max_len, uint32_t info[4]) {
  if (rplgpu_nav_field_check(f) != RPLGPU_OK || !grid || !potential || !path || !info || max_len == 0)
    return RPLGPU_ERR_INVALID_ARG;
  const Grid g{f, grid, (int)f->width, (int)f->height};
  const uint64_t cells = (uint64_t)f->width * f->height;
  uint32_t len = 0, flags = 0, d0 = RPLGPU_NAV_UNREACHED, last = start;
  if (start >= cells) {
    flags = RPLGPU_NAV_PATH_NO_START;
  } else if ((d0 = potential[start]) == RPLGPU_NAV_UNREACHED) {
    flags = RPLGPU_NAV_PATH_UNREACHED;
  } else {
    uint32_t c = start;
    for (;;) {
      path[len++] = c;
      last = c;
      const uint32_t d = potential[c];
      if (d == 0) {
        flags = RPLGPU_NAV_PATH_REACHED;
        break;
      }
      if (len == max_len) {
        flags = RPLGPU_NAV_PATH_TRUNCATED;
        break;
      }
      const int cx = (int)(c % f->width), cy = (int)(c / f->width);
      int taken = -1;
      for (int dir = 0; dir < 8 && taken < 0; ++dir) {
        if (!g.allowed(cx, cy, dir)) continue;
        const uint32_t dn = potential[(size_t)(cy + kDy[dir]) * f->width + (size_t)(cx + kDx[dir])];
        if (dn != RPLGPU_NAV_UNREACHED &&
            (uint64_t)dn + (uint64_t)(dir < 4 ? 5u : 7u) * g.weight(cx, cy) == (uint64_t)d)
          taken = dir;
      }
      if (taken < 0) {
        flags = RPLGPU_NAV_PATH_BROKEN;
        break;
      }
      c = (uint32_t)((size_t)(cy + kDy[taken]) * f->width + (size_t)(cx + kDx[taken]));
    }
  }
  info[0] = len;
  info[1] = flags;
  info[2] = d0;
  info[3] = last;
  return (int32_t)flags;
}

}  // extern "C"
