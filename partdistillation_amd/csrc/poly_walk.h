// The arithmetic of the polygon rasteriser (polygon.hip, include/pd_poly.h), one boundary position at a time: plain C++ that compiles for
// the device and for the host, so the same lines can be run under a host sanitizer or against a serial restatement without a GPU.
#ifndef PD_POLY_WALK_H
#define PD_POLY_WALK_H
#include <stdint.h>

#ifdef __HIPCC__
#define PD_POLY_HD __host__ __device__ __forceinline__
#else
#define PD_POLY_HD inline
#endif

// the serial original is compiled without fused multiply-add: `start + slope * t` must round twice here too (a fused form changes
// tables: tests/test_polygon_raster_gpu.py has the triangles).  Holds for the rest of the translation unit that includes this.
#pragma clang fp contract(off)

constexpr double POLY_COORD_MAX = 1073741823.0;                           // 2^30 - 1: differences of two coordinates fit an int

PD_POLY_HD int poly_floor_div5(int a) { return a / 5 - (a % 5 < 0); }

// (int)(5 * x + .5), C truncation; clamped so that nothing downstream overflows, NaN -> 0
PD_POLY_HD int poly_upsample(double x)
{
  double v = 5.0 * x + .5;
  if (!(v == v)) v = 0.0;
  v = v < -POLY_COORD_MAX ? -POLY_COORD_MAX : (v > POLY_COORD_MAX ? POLY_COORD_MAX : v);
  return (int)v;
}

// the walk's (int)(start + slope * t + .5)
PD_POLY_HD int poly_point(int start, double slope, int t) { return (int)((double)start + slope * (double)t + .5); }

// An edge between the upsampled points (x0, y0) -> (x1, y1) crosses from column 5 X + 2 to 5 X + 3 once for every X in [0, w - 1] with
// min(x0, x1) <= 5 X + 2 <= max(x0, x1) - 1: the columns first .. first + count - 1.  (Along the walk the column moves monotonically and by
// at most one per step; a zero-length edge has count 0.)
struct PolyColumns { int first, count; };

PD_POLY_HD PolyColumns poly_edge_columns(int x0, int x1, int w)
{
  const int lo = x0 < x1 ? x0 : x1, hi = x0 < x1 ? x1 : x0;
  const int n_lo = poly_floor_div5(lo + 2), n_hi = poly_floor_div5(hi - 3);          // ceil((lo - 2) / 5), floor((hi - 1 - 2) / 5)
  PolyColumns c;
  c.first = n_lo > 0 ? n_lo : 0;
  c.count = (n_hi < w - 1 ? n_hi : w - 1) - c.first + 1;
  if (c.count < 0) c.count = 0;
  return c;
}

// What the walk of an edge needs: start / end after the original's swap and the slope.  Only for an edge with a crossing (x0 != x1), so
// the divisor is never zero; the division is paid by whoever computes crossings of the edge, not by whoever only counts them.
struct PolyEdge {
  int xs, ys, xe, dy;
  bool shallow;
  double slope;
};

PD_POLY_HD PolyEdge poly_edge(int x0, int y0, int x1, int y1)
{
  PolyEdge e;
  const int dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
  e.shallow = dx >= dy;
  const bool swap = e.shallow ? x0 > x1 : y0 > y1;
  e.xs = swap ? x1 : x0; e.ys = swap ? y1 : y0; e.xe = swap ? x0 : x1; e.dy = dy;
  const int ye = swap ? y0 : y1;
  e.slope = e.shallow ? (double)(ye - e.ys) / dx : (double)(e.xe - e.xs) / dy;
  return e;
}

// the boundary position X * h + row of the edge's crossing of column X (one of the edge's columns)
PD_POLY_HD int poly_crossing(const PolyEdge &e, int X, int h)
{
  const int m = 5 * X + 2;
  int vmin;
  if (e.shallow) {                                                        // the points t and t + 1 have the columns m and m + 1
    const int t = m - e.xs, a = poly_point(e.ys, e.slope, t), b = poly_point(e.ys, e.slope, t + 1);
    vmin = a < b ? a : b;
  } else {                                                                // bisection for the first step at which the column has left m
    const bool rising = e.xe > e.xs;                                      // (rising) or reached it (falling); the rows are ys + t
    int lo = 0, hi = e.dy;
    while (hi - lo > 1) {
      const int mid = lo + ((hi - lo) >> 1);
      const int u = poly_point(e.xs, e.slope, mid);
      if (rising ? u > m : u <= m) hi = mid; else lo = mid;
    }
    vmin = e.ys + hi - 1;                                                 // the smaller row of the steps hi - 1 and hi
  }
  const int row = vmin <= 2 ? 0 : (((vmin + 2) / 5) < h ? (vmin + 2) / 5 : h);         // clamp(ceil((vmin + .5) / 5 - .5), 0, h)
  return X * h + row;
}
#endif
