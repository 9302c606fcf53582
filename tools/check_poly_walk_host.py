"""Runs the polygon rasteriser's arithmetic (partdistillation_amd/csrc/poly_walk.h, the lines the kernel of csrc/polygon.hip executes per
boundary position) on the HOST under AddressSanitizer and UBSan and compares every table with the serial restatement of
tests/poly_oracle.py and with the host's exact table sizes (functions/polygon.polygon_tables).  No GPU.  Builds
tools/probes/poly_walk_host.cpp with the clang++ of the ROCm installation (HOST_CXX overrides it) into a temporary directory.
    python tools/check_poly_walk_host.py [--polygons 1500]"""
import argparse, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import poly_oracle as P
from partdistillation_amd.functions.polygon import polygon_tables

ap = argparse.ArgumentParser()
ap.add_argument("--polygons", type=int, default=1500, help="random polygons on small canvases (60 more on canvases of 300..900 px)")
args = ap.parse_args()
cxx = os.environ.get("HOST_CXX", "/opt/rocm/llvm/bin/clang++")
rng = np.random.RandomState(5)
cases = [(np.asarray(p, dtype=np.float64), h, w) for p, h, w in
         (([2, 3, 2, 9, 11, 9, 11, 3], 12, 15), ([-5, -5, 60, -5, 60, 60, -5, 60], 20, 30), ([3, 3, 3, 3, 3, 3], 10, 10),
          ([1, 1, 8, 1, 8, 8, 1, 1], 10, 10))]
cases += [((np.asarray(t, dtype=np.float64) / 5).reshape(-1), 24, 24) for t in P.CONTRACTION_TRIANGLES]
for i in range(args.polygons):
    k, (h, w) = rng.randint(3, 9), rng.randint(1, 40, 2)
    poly = (rng.uniform(-8, 48, 2 * k), rng.randint(-8, 49, 2 * k).astype(np.float64), rng.randint(-16, 97, 2 * k) / 2.0,
            rng.uniform(-300, 300, 2 * k))[i % 4]
    cases.append((poly, int(h), int(w)))
for i in range(60):
    k, (h, w) = rng.randint(3, 6), rng.randint(300, 900, 2)
    cases.append((rng.uniform(-100, 1000, 2 * k), int(h), int(w)))
text = f"{len(cases)}\n" + "".join(f"{h} {w} {len(p) // 2} " + " ".join(repr(float(v)) for v in p) + "\n" for p, h, w in cases)
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "poly_walk_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "partdistillation_amd", "csrc"), os.path.join(ROOT, "tools", "probes", "poly_walk_host.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
if out.returncode != 0:
    sys.exit(f"poly_walk_host failed (rc {out.returncode}):\n{out.stderr[-3000:]}")
bad = 0
for (p, h, w), line in zip(cases, out.stdout.strip().split("\n")):
    got, want = np.asarray(line.split(), dtype=np.int64), P.table(p, h, w)
    if not (len(got) == len(want) == polygon_tables([p], h, w)[2][1] and np.array_equal(got, want)):
        bad += 1
        print("MISMATCH", p.tolist(), h, w)
print(f"{len(cases)} polygons under AddressSanitizer + UBSan, {bad} tables differ from the serial restatement")
sys.exit(1 if bad else 0)
