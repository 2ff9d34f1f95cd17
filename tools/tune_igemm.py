"""Tile-config sweep for the fp32 weight gradient (tuning aid, diagnostic build): runs tools/bench_kernels.py under
VRNET_WGRAD_CFG=0,1 (128-wide, 64 x 64 tiles) in child processes and prints, per weight-gradient shape, the time of each config.
    VRNET_HIP_LIB=asy-vrnet_amd/csrc/libvrnet_hip_tuning.so python tools/tune_igemm.py [--wgrad] [bench_kernels.py args]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = [a for a in sys.argv[1:] if a != "--wgrad"]     # (the only sweep left; the flag is accepted as before)
res = {}
for cfg in (0, 1):
    env = dict(os.environ, VRNET_WGRAD_CFG=str(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_kernels.py")] + args, env=env,
                         capture_output=True, text=True).stdout
    for line in out.splitlines():
        if line.startswith("#") or not line.strip() or "amdgpu" in line:
            continue
        f = line.split()
        if f[5] != "2":
            continue
        res.setdefault(" ".join(f[5:]), {})[cfg] = (float(f[2]), int(f[1]), float(f[3]))
rows = []
for key, d in res.items():
    if len(d) < 2:
        continue
    best = min(d, key=lambda c: d[c][0])
    rows.append((d[best][0] * d[best][1], key, d, best))
rows.sort(reverse=True)
tot = {c: sum(d[c][0] * d[c][1] for _, _, d, _ in rows) for c in (0, 1)}
print("# totals us/step per forced config:", tot, "best-of:", sum(r[0] for r in rows))
print("# key = mode B H W Cin OH OW Cout k s d act res ypre aux nchw | us cfg0 cfg1 | best | M N K")
for t, key, d, best in rows:
    f = key.split()
    mode, B, H, W, Ci, OH, OW, Co = map(int, f[:8])
    M = B * H * W
    print(f"{key:60s} | {d[0][0]:8.1f} {d[1][0]:8.1f} | {best} | M={M} N={Ci} K={Co} x{d[0][1]}")
