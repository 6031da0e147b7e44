"""How the contract kernel (C2: EQ, d = 3, n = 131072, fp32, all entries) fills and drains the chip, from the clock stamps of its diagnostic build
(option mfma_stamp: per workgroup the shader clock and the 100 MHz counter at the start and end of its column loop; covgram_ctx_read_stamps).

Per stamped launch, on the 100 MHz counter (common to the whole chip; 10 ns steps):
  covered   slot-time inside workgroup lifetimes / (kernel duration x resident slots); duration = first start .. last end
  ramp      slot-time before the first workgroup of each slot starts (the first `slots` starts against the earliest)
  tail      slot-time between a slot's last end and the kernel's end, counted from the last START on (nothing is left to hand out then)
  turnover  the rest: the gaps between one workgroup's end and the start of the next on the same slot (epilogue, dispatch, prologue)
  and the time from the first workgroup's end to the last one's, from the last start to the last end, and the durations by chunk length.
Usage: c2_drain_probe.py [--graded -1|0|1|2|3] [--launches 5] [--rows N]   (--rows: a row shard of the same columns)"""
import argparse, ctypes as C, os, sys, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "covariancefunctions.jl_amd"))
import covgram as cg

ap = argparse.ArgumentParser()
ap.add_argument("--graded", type=int, default=None, help="option mfma_graded (default: the library's; ignored by a build without the option)")
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--rows", type=int, default=131072)
args = ap.parse_args()

n, d = 131072, 3
rng = np.random.default_rng(0xC0F + 1)
X = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda(); a = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
cg.set_option("mfma_sym", 0)
if args.graded is not None:
    try: cg.set_option("mfma_graded", args.graded)
    except Exception as e: print(f"(mfma_graded not set: {e})")
G = cg.gramian(cg.EQ(), X[:args.rows].contiguous(), X); y = torch.empty(args.rows, dtype=torch.float32, device="cuda")
for _ in range(10): G.mul_(y, a)
torch.cuda.synchronize()
e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): G.mul_(y, a)
e1.record(); e1.synchronize()
inst = cg.get_info("last_mfma_instance")
try: graded = cg.get_info("last_mfma_graded")
except Exception: graded = 0
print(f"rows {args.rows} x cols {n}, d = {d}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per MVM (product build), instance {inst}, graded chunks {graded}")

lib, h = cg._ffi.lib(), cg.get_ctx().handle
wpb = inst // 1000 % 10
slots = cg.get_info("num_cus") * 16 // wpb          # 4 waves per SIMD (the LDS-shared instances at d <= 4: amdgpu_waves_per_eu), 16 per CU
cg.set_option("mfma_stamp", 1)
rows = []
for launch in range(args.launches + 1):
    G.mul_(y, a)
    cnt = C.c_int64(0)
    cg._ffi.check(lib.covgram_ctx_read_stamps(h, None, 0, C.byref(cnt)))
    if cnt.value == 0: sys.exit("no stamped launch: this shape does not run a stamped instance")
    buf = (C.c_uint64 * (4 * cnt.value))()
    cg._ffi.check(lib.covgram_ctx_read_stamps(h, buf, cnt.value, C.byref(cnt)))
    if launch == 0: continue                          # (the first stamped launch sizes the stamp buffer)
    s = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).astype(np.int64)
    r0, r1 = s[:, 1], s[:, 3]
    t0, t1 = r0.min(), r1.max()
    span, life = float(t1 - t0), (r1 - r0).astype(np.float64)
    nslot = min(slots, len(s))
    covered = life.sum() / (span * nslot)
    ramp = float((np.sort(r0)[:nslot] - t0).sum()) / (span * nslot)
    last_start = r0.max()
    tail = float((t1 - np.maximum(np.sort(r1)[-nslot:], last_start)).sum()) / (span * nslot)
    khz = np.median((s[:, 2] - s[:, 0]) / np.maximum(life, 1.0)) * 1e5
    rows.append((span / 100, covered, ramp, tail, (t1 - r1.min()) / 100, (t1 - last_start) / 100, khz / 1e6))
    print(f"launch {launch}: {len(s)} workgroups on {nslot} slots, duration {span / 100:.1f} us, clock {khz / 1e6:.3f} GHz: covered {covered:.4f}, ramp {ramp:.4f}, "
          f"tail {tail:.4f}, turnover {1 - covered - ramp - tail:.4f}; first end -> last end {(t1 - r1.min()) / 100:.1f} us, last start -> last end {(t1 - last_start) / 100:.1f} us")
cg.set_option("mfma_stamp", 0)
m = np.median(np.array(rows), axis=0)
print(f"median of {len(rows)} launches: duration {m[0]:.1f} us, covered {m[1]:.4f}, ramp {m[2]:.4f}, tail {m[3]:.4f}, turnover {1 - m[1] - m[2] - m[3]:.4f}, "
      f"first end -> last end {m[4]:.1f} us ({m[4] / m[0]:.3f} of the duration), last start -> last end {m[5]:.1f} us ({m[5] / m[0]:.3f}), clock {m[6]:.3f} GHz")
# workgroup durations of the last launch, by chunk (launch order is chunk-major: workgroup = chunk * row blocks + row block)
rb = (args.rows + 64 * wpb - 1) // (64 * wpb)
print("durations of the last launch by chunk (us): chunk: min / 5 % / median / 95 % / max, and the median start")
for c in range(len(s) // rb):
    q = life[c * rb:(c + 1) * rb] / 100
    print(f"  chunk {c:2d}: {q.min():7.1f} {np.percentile(q, 5):7.1f} {np.median(q):7.1f} {np.percentile(q, 95):7.1f} {q.max():7.1f}   start {np.median(r0[c * rb:(c + 1) * rb] - t0) / 100:7.1f}")
