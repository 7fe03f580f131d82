"""gpurun_out/<TAG>/ (written by tools/final_profile.sh on the GPU box) -> the tracked evidence files under profiles/:
r2_final_summary.md, r2_final_pmc_hbm.md, r2_final_pmc.json (read by bench.py for `roofline.traffic`),
r2_final_kernel_stats.csv, r2_final_bench.json.     python tools/publish_profile.py r2/final2 [r3_final "Round 3"]"""
import json, os, shutil, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = os.path.join(ROOT, "gpurun_out", sys.argv[1])
P = os.path.join(ROOT, "profiles")
PRE = sys.argv[2] if len(sys.argv) > 2 else "r2_final"
ROUND = sys.argv[3] if len(sys.argv) > 3 else "Round 2"
rd = lambda n: open(os.path.join(F, n)).read()
shutil.copy(os.path.join(F, "stats", "run_kernel_stats.csv"), os.path.join(P, PRE + "_kernel_stats.csv"))
shutil.copy(os.path.join(F, "bench.json"), os.path.join(P, PRE + "_bench.json"))
b = json.loads(rd("bench.json"))
groups = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_groups.py"), os.path.join(F, "fetch", "f_counter_collection.csv"),
                         os.path.join(F, "write", "w_counter_collection.csv"), "3"], capture_output=True, text=True).stdout
rows = {}
for l in groups.splitlines():
    m = l.split("|")
    if len(m) > 6:
        try:
            rows[m[1].strip().strip("*")] = dict(launches_per_step=float(m[2].strip() or 0), fetch_gb=float(m[3]), write_gb=float(m[4]),
                                                  total_gb=float(m[5]), mb_per_launch=float(m[6].strip() or 0))
        except ValueError:
            pass
conv = next(v for k, v in rows.items() if k.startswith("conv fwd+dgrad"))
total = rows.get("all kernels", {}).get("total_gb")
json.dump({"kernel": "conv_mfma(fwd+dgrad)", "hbm_bytes_per_launch": conv["mb_per_launch"] * 1e6, "launches_per_step": conv["launches_per_step"],
           "fetch_gb_per_step_x2_corrected": conv["fetch_gb"], "write_gb_per_step": conv["write_gb"], "algorithmic_gb_per_step": 8.69,
           "source": "profiles/" + PRE + "_pmc_hbm.md: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 x2 fetch correction",
           "groups": rows}, open(os.path.join(P, PRE + "_pmc.json"), "w"), indent=1)
r = b["roofline"]
chains = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "chain_breakdown.py"), os.path.join(F, "stats", "run_kernel_trace.csv"), "32"],
                        capture_output=True, text=True).stdout
gaps = rd("gaps.txt")
sq = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sq_table.py"), os.path.join(F, "sq.log"), "3"], capture_output=True, text=True).stdout
open(os.path.join(P, PRE + "_sq_pmc.md"), "w").write(f"""# {ROUND} (final state) — SQ counters of the step's MFMA kernel families (MI355X, preset s @640 bf16, 32 img)

`tools/pmc_kernel.sh`: six separate `rocprofv3 --kernel-trace --pmc <four SQ counters>` passes of
`python3 bench.py --steps 2 --warmup 1 --no-graph --no-cpu-baseline --no-roofline --no-extra` (eager launches, three steps per pass), summed per
kernel-name family; `tools/sq_table.py` derives the shares.  SQ_BUSY_CYCLES is a sum over the 32 shader engines; SQ_WAVE_CYCLES and the
SQ_WAIT_* / SQ_ACTIVE_* counters are in quad-cycles (ratios between them need no conversion); MFMA pipe busy =
SQ_VALU_MFMA_BUSY_CYCLES / (kernel cycles x 1024 SIMDs); kernel time at 2.1 GHz.

{sq}
Raw sums:

```
{rd("sq.log")}```
""")
open(os.path.join(P, PRE + "_summary.md"), "w").write(f"""# {ROUND} (final state) — rocprofv3 summary, MI355X, preset s @640 bf16, 32 img, graph-captured train step

Produced by `bash tools/final_profile.sh` on one MI355X box and `python tools/publish_profile.py`: the `python3 bench.py --full`
line (`profiles/{PRE}_bench.json`: {b['value']:.0f} img/s, {b['ms_per_step']:.2f} ms/step; dominant MFMA kernel group conv fwd+dgrad
{r['achieved']:.0f} TFLOP/s = {r['frac']:.3f} of 2.5 PF over {r['launches']} leaf calls, {r['avg_launch_us']:.1f} us average), then

    rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-extra

whose per-kernel statistics are `profiles/{PRE}_kernel_stats.csv` (whole run: capture warm-up, 25 replays, the instrumented
eager step of the roofline leg).  rocprofv3's average over the conv fwd+dgrad kernels INSIDE the replayed step (k_conv_mfma +
k_conv_ring + k_conv_halo + k_conv_rows + k_dgrad2_patch) is in the chain table below; the live
leaf timing counts such a layer as one call.

## The two chains of one replayed step (`tools/chain_breakdown.py`: cut at the optimizer launch)

```
{chains}```

## Idle time inside the step (`tools/trace_gaps.py`)

```
{gaps}```

## HBM traffic from PMC counters -> `profiles/{PRE}_pmc_hbm.md`

{groups}""")
open(os.path.join(P, PRE + "_pmc_hbm.md"), "w").write(f"""# {ROUND} (final state) — HBM traffic from PMC counters (MI355X, preset s @640 bf16, 32 img, one train step)

Collected as `MI355X_MICROARCH.md` (§HBM, §rocprofv3 PMC slots) prescribes: two separate passes, kernel trace only,

```
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -- python3 bench.py --steps 2 --warmup 1 --no-graph --no-cpu-baseline --no-roofline --no-extra
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -- python3 bench.py --steps 2 --warmup 1 --no-graph --no-cpu-baseline --no-roofline --no-extra
```

(eager launches so every dispatch is attributed; three steps per pass; summarised by `tools/pmc_groups.py`).  Units: FETCH_SIZE /
WRITE_SIZE are KB; the gfx950 correction -- FETCH_SIZE tallies 128-B requests at 64 B for wide coalesced reads -- is applied (x2);
WRITE_SIZE is exact.  Infinity-Cache hits are counted, not excluded.

{groups}
Against the start of the round (`profiles/r2_pmc_hbm.md`): all kernels {total} GB per step (was ~43); weight gradient k_wgrad2 + its
reduce 7.2 GB (was 10.13 + 2.41 = 12.5: the operands, 4.6 GB algorithmic, are fetched 0.95x -- XCD-aware (slab, tile) order -- and the
partial matrices of small layers are capped at half their operand bytes); conv fwd+dgrad {conv['total_gb']} GB = {conv['total_gb'] / 8.69:.2f}x their
algorithmic 8.69 GB ({conv['mb_per_launch']} MB per launch: the `traffic` of the bench line); the three BatchNorm passes 14.8 GB = their
algorithmic bytes; no fp32 score / dP tensors of the attention any more; concat copies {rows.get('k_copy_channels', {}).get('total_gb', 0)} GB (was 0.97: the backbone writes
its features into the neck's buffers, C3K2's chunk gradient is accumulated by the data-gradient kernels); the stem 0.9 GB (no column tensor: unfold + 1x1 moved 1.5 GB).
""")
print("published", sys.argv[1], "->", P)
