// Host harness of partdistillation_amd/csrc/poly_walk.h (the arithmetic of the polygon rasteriser, which compiles for host and device):
// a stand-alone program, no GPU, meant to be built with -fsanitize=address,undefined by tools/check_poly_walk_host.py, which compares
// its tables with the serial restatement of tests/poly_oracle.py.
// stdin: "n", then per polygon "h w k x0 y0 x1 y1 ...";  stdout: per polygon its table (0, then the boundary positions ascending).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "poly_walk.h"

int main()
{
  int n;
  if (scanf("%d", &n) != 1) return 1;
  for (int i = 0; i < n; ++i) {
    int h, w, k;
    if (scanf("%d %d %d", &h, &w, &k) != 3 || k < 1) return 1;
    std::vector<double> xy(2 * (size_t)k);
    for (double &v : xy)
      if (scanf("%lf", &v) != 1) return 1;
    std::vector<int> a;
    for (int j = 0; j < k; ++j) {
      const int jn = (j + 1) % k;
      const int x0 = poly_upsample(xy[2 * j]), y0 = poly_upsample(xy[2 * j + 1]);
      const int x1 = poly_upsample(xy[2 * jn]), y1 = poly_upsample(xy[2 * jn + 1]);
      const PolyColumns c = poly_edge_columns(x0, x1, w);
      if (c.count == 0) continue;
      const PolyEdge e = poly_edge(x0, y0, x1, y1);
      for (int q = 0; q < c.count; ++q) a.push_back(poly_crossing(e, c.first + q, h));
    }
    std::sort(a.begin(), a.end());
    printf("0");
    for (int v : a) printf(" %d", v);
    printf("\n");
  }
  return 0;
}
