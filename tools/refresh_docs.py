#!/usr/bin/env python3
"""Rewrite the CHECKED statements of README.md (headline block) and profiles/README.md (the latest round's <!-- check:rNN --> row) from the recorded files
profiles/rNN_bench_n1.json + rNN_bench_kernel_stats.csv, so that tests/test_host.py::test_docs_quote_the_recorded_numbers holds by construction.
usage: python tools/refresh_docs.py [rNN]   (default: the latest record)"""
import csv, glob, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rnd = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_n1.json")))[-1])[:3]
line = json.loads([x for x in open(os.path.join(ROOT, "profiles", f"{rnd}_bench_n1.json")) if x.startswith("{")][0])
rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", f"{rnd}_bench_kernel_stats.csv"))))
r = line["roofline"]
inst = r.get("kernel_instance") or "dense_mfma_eq_kernel<1, 2, 8, 1, 0, 1>"
k = [x for x in rows if inst.replace("covgram::", "") in x["Name"]][0]
ks = [x for x in rows if "dense_mfma_sym2_kernel<1001, 1, 8" in x["Name"]]
c = line["configs"]
block = f"""<!-- headline:begin -->
* contract run (C2: EQ, d = 3, n = 131072, fp32, ALL n·m entries, `bench.py` `value`): **{line['value']:.1f} MVM/s**, {line['ms_per_step']:.3f} ms per step, kernel {r['kernel_avg_ms']:.3f} ms,
  `roofline.frac` {r['frac']:.3f}, `issue_roofline_frac` {r['issue_roofline_frac']:.3f}; rocprofv3 average of the same kernel under the profiler {float(k['AverageNs']) * 1e-6:.3f} ms over {int(k['Calls'])} dispatches
* the same product on the library's default path for gramian(EQ, x) (upper triangle once, `symmetric_variant`): {line['symmetric_variant']['value']:.1f} MVM/s, {line['symmetric_variant']['ms_per_step']:.3f} ms per step
* the reference's own arithmetic (direct differences in fp32, `direct_difference_variant`): {line['direct_difference_variant']['value']:.1f} MVM/s
* CPU restatement of `src/gramian.jl:78-87` on the box's {line['cpu_baseline']['cores']} host threads (`cpu_baseline`): {line['cpu_baseline']['value']:.3f} MVM/s
<!-- headline:end -->"""
p = os.path.join(ROOT, "README.md"); s = open(p).read()
s = re.sub(r"<!-- headline:begin -->.*?<!-- headline:end -->", lambda m: block, s, flags=re.S)
open(p, "w").write(s)
row = (f"| `{rnd}_bench_n1.json`, `{rnd}_bench_kernel_stats.csv` | <!-- check:{rnd} --> `python3 bench.py --full --steps 20 --warmup 5` on one MI355X at the end of round {int(rnd[1:])} and "
       f"`rocprofv3 --kernel-trace --stats` of `bench.py` (`tools/profile_bench.sh`): the contract kernel is unchanged, `{inst}`, all n·m entries — contract run {line['value']:.1f} MVM/s, "
       f"live `kernel_avg_ms` {r['kernel_avg_ms']:.3f}, profiled average {float(k['AverageNs']) * 1e-6:.3f} ms over {int(k['Calls'])} dispatches (the profiler lowers the clock; cold dispatches included), "
       f"`roofline.frac` {r['frac']:.2f}; `roofline.traffic` taken only from a PMC pass of the launched instance (`traffic_check`), row-wise errors beside the norm-wise ones; "
       f"`symmetric_variant` {line['symmetric_variant']['value']:.0f} MVM/s on `dense_mfma_sym2_kernel<1001, 1, 8>`" + (f" ({float(ks[0]['AverageNs']):.0f} ns profiled average)" if ks else "") +
       f"; `configs`: C1 {c['C1']['ms'] * 1e3:.1f} µs, C3 shard {c['C3_shard']['ms']:.2f} ms, C3 symmetric partial {c['C3_sym_partial']['ms']:.2f} ms, C4 {c['C4']['ms']:.2f} ms, C5 {c['C5']['ms'] * 1e3:.1f} µs, "
       f"`F2_composite` {c['F2_composite']['ms']:.2f} ms, `F2_sum_of_three` {c['F2_sum_of_three']['ms']:.2f} ms in one pass against {c['F2_sum_of_three']['ms_one_mvm_per_term']:.2f} "
       f"(secondary configs vary ±5 % between boxes) |")
p = os.path.join(ROOT, "profiles", "README.md"); s = open(p).read()
s2 = re.sub(r"^\| `" + rnd + r"_bench_n1\.json`[^\n]*<!-- check:" + rnd + r" -->[^\n]*$", lambda m: row, s, flags=re.M)
assert s2 != s or row in s, "no checked row for " + rnd
open(p, "w").write(s2)
print("refreshed from", rnd)
