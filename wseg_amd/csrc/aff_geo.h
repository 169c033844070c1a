// aff_geo.h — the AffinityNet pair geometry (tool/pyutils.py get_indices_of_pairs) shared by affinity.hip and aff_loss.hip: one copy.
// Not in common.h: every conv / wgrad file includes that header and none of them walks pairs.
#pragma once
#include "common.h"

namespace {

struct AffGeo {
  int P, h, w, r, cw, n_from;
  int dy[WSEG_AFF_MAX_OFFSETS], dx[WSEG_AFF_MAX_OFFSETS];
};

// the reference's offset order (tool/pyutils.py get_indices_of_pairs)
int aff_offsets(int r, int* dy, int* dx) {
  if (r < 2 || r > 6) return -1;
  int n = 0;
  for (int x = 1; x < r; ++x) { if (dy) { dy[n] = 0; dx[n] = x; } ++n; }
  for (int y = 1; y < r; ++y)
    for (int x = -r + 1; x < r; ++x)
      if (x * x + y * y < r * r) { if (dy) { dy[n] = y; dx[n] = x; } ++n; }
  return n;
}

int aff_geo(int h, int w, int r, AffGeo& g) {
  WSEG_CHECK(r >= 2 && r <= 6, "aff: radius %d outside [2, 6] (the reference's pair set is empty below 2)", r);
  WSEG_CHECK(h >= r && w >= 2 * r - 1, "aff: a %dx%d map has no 'from' pixel at radius %d", h, w, r);
  g.P = aff_offsets(r, g.dy, g.dx);
  g.h = h; g.w = w; g.r = r;
  g.cw = w - 2 * (r - 1);
  g.n_from = (h - r + 1) * g.cw;
  return 0;
}

}  // namespace
