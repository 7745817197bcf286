#!/usr/bin/env python3
"""Fills the @@R6_...@@ placeholders of tools/design/DESIGN.in.md from the committed profiles of the round and runs
tools/make_design.py.  The numbers in DESIGN.md are therefore the ones in profiles/: usage  python tools/fill_design.py r06

KNOWN DRIFT, to be settled before the next regeneration: the committed DESIGN.md carries text on the pipelined solver's tail
behind the separator (section 5.1's penta_pipe row, 5.2's "Joiners" / "Producers: closed form" items, its timeline and bound,
the numbers table's closed_tail row, item 8 of section 10) that was written into DESIGN.md alone; tools/design/DESIGN.in.md and
this script do not produce it, so a regeneration drops it.  Sections 14.4 and 14.5 are in both."""
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = sys.argv[1] if len(sys.argv) > 1 else "r06"
P = lambda f: os.path.join(ROOT, "profiles", f"{R}_{f}")


def avg_us(path, kernel):
    for row in csv.DictReader(open(path)):
        if kernel in row["Name"]:
            return float(row["AverageNs"]) / 1e3
    raise SystemExit(f"{kernel} not in {path}")


def small_iter_table():
    """profiles/<round>_small_iteration_times.txt as a table: us per iteration by launch structure"""
    t = {}
    for m in re.finditer(r"(\w+) constraints (off|enforced) tr_small=(\d) tr_fold=(\d): ([\d.]+) ms", open(P("small_iteration_times.txt")).read()):
        t.setdefault((m.group(1), m.group(2)), {})[(m.group(3), m.group(4))] = 1e3 * float(m.group(5))
    rows = ["| µs per iteration (N = 40, scaling on) | ONE launch (`tr_fold`) | two: `tr_iter_kernel` + `gn_small_kernel` | the loop of 4 / 7 launches |", "|---|---|---|---|"]
    for (name, con), v in t.items():
        rows.append(f"| {name}, constraint {con} | **{v[('1', '1')]:.1f}** | {v[('1', '0')]:.1f} | {v[('0', '0')]:.1f} |")
    return "\n" + "\n".join(rows) + "\n"


b = json.load(open(P("bench.json")))
lm = json.load(open(P("latency_model.json")))
tr = json.load(open(P("pmc_traffic.json")))
cfgs = open(P("all_configs.txt")).read()
fd_us, pipe_us = avg_us(P("kernel_stats.csv"), "fd_kernel"), avg_us(P("kernel_stats.csv"), "penta_pipe_kernel")
pipe_alone = avg_us(P("kernel_stats_assembly_in_its_own_launch.csv"), "penta_pipe_kernel")
fdm, pm, p8 = lm["fd_kernel"], lm["penta_pipe_kernel"], lm["penta_pipe8_predicted"]
traffic = (tr["penta_pipe_kernel"]["fetch_bytes_per_launch_x2"] + tr["penta_pipe_kernel"]["write_bytes_per_launch_raw"]) / 1e6
gbs = 2259440 / pipe_us / 1e3
cpu = b["cpu_baseline"]
m = lambda pat: re.search(pat, cfgs)
tl = [l.rstrip() for l in open(P("nd_timeline_gn_step.txt")) if re.match(r"(P0|P3|J1|J2|separator  )", l) or "chains saw" in l or "block row 1 part 0" in l]
fi = dict(re.findall(r"(\w+): ([\d.]+) ms/iteration", open(P("full_iteration_times.txt")).read()))
mpc = re.search(r"mini_cheetah: N=20.*?median ([\d.]+) ms, p10 ([\d.]+), p90 ([\d.]+)", open(P("mpc_latency.txt")).read())
numbers = f"""| | |
|---|---|
| Gauss-Newton iterations / s, one problem (`value`) | **{b['value']:.0f}** ({1e3 * b['ms_per_step']:.1f} µs a step; round 5: 12,358, round 4: 11.9k, round 3: 10.5k, round 2: 8.3k, round 1: 6.2k) |
| kernels, rocprofv3 averages (`profiles/{R}_kernel_stats.csv`) | `fd_kernel<3,3>` {fd_us:.2f} µs, `penta_pipe_kernel<19>` {pipe_us:.2f} µs with the assembly inside ({pipe_alone:.2f} alone: `..._assembly_in_its_own_launch.csv`); HIP events {1e3 * b['roofline']['all_kernels_avg_ms']['fd_kernel']:.1f} + {1e3 * b['roofline']['all_kernels_avg_ms']['penta_pipe_kernel']:.1f} |
| one step, synchronised before and after | median {1e3 * b['step_latency_ms']['median']:.1f} µs (p10 {1e3 * b['step_latency_ms']['p10']:.1f}, p90 {1e3 * b['step_latency_ms']['p90']:.1f}) |
| `roofline` (the solver's launch) | {b['roofline']['achieved']:.1f} GB/s algorithmic = {b['roofline']['frac']:.4f} of 8 TB/s; counter traffic {traffic:.2f} MB a launch = {traffic * 1e6 / 2259440:.2f} × the algorithmic bytes |
| CPU port on the box's host cores (`cpu_baseline`, {cpu['iterations_per_repeat']} iterations × {cpu['repeats']}, median) | {", ".join(f"{t} threads: {v:.0f} it/s (spread {100 * (cpu['spread_by_num_threads'].get(t) or 0):.0f} %)" for t, v in cpu['iters_per_s_by_num_threads'].items())}; best leg {cpu['value']:.0f} ⇒ **{b['speedup_vs_cpu_baseline']:.1f} ×** (the ratio moves with the host: the same command gave 209 / 392 / 461 / 486 it/s in `{R}_all_configs.txt`, i.e. {b['value'] / 486:.0f} ×) |
| batch of 16 / 64 problems, one host thread | {b['batch_mode'][0]['value'] / 1e3:.0f}k / {b['batch_mode'][1]['value'] / 1e3:.0f}k it/s aggregate |
| full trust-region iteration (`TrajectoryOptimizer::Solve`, the YAML's settings) | {b['full_iteration']['ms_per_iteration']:.3f} ms (CPU port {b['full_iteration']['cpu_port_ms_per_iteration']:.2f} ms) |
| MPC re-plan (cheetah N = 20, `idto_mpc_update`) | median {b['mpc_replan']['ms_per_replan_median']:.3f} ms |"""
vals = {
    "R6": R, "R6_FD_US": f"{fd_us:.1f}", "R6_PIPE_US": f"{pipe_us:.1f}", "R6_PIPE_ALONE_US": f"{pipe_alone:.1f}",
    "R6_STEP_US": f"{1e3 * b['ms_per_step']:.1f}", "R6_ITS": f"{b['value']:.0f}",
    "R6_FD_VALU": f"{fdm['valu_instructions_per_wavefront']:,}", "R6_FD_WAIT": f"{100 * fdm['wait_frac_of_wave_cycles']:.0f} %",
    "R6_FD_ACTIVE": f"{100 * fdm['valu_active_frac_of_wave_cycles']:.0f} %", "R6_FD_FLOOR": f"{fdm['issue_floor_us']:.1f}",
    "R6_FD_FRAC": f"{fdm['achieved_frac_of_issue_floor']:.2f}",
    "R6_FD44_US": m(r"allegro_hand N=60:.*?fd_kernel ([\d.]+)").group(1),
    "R6_ASM_US": m(r"allegro_hand N=60:.*?assemble_terms_kernel ([\d.]+)").group(1),
    "R6_ND23_US": m(r"allegro_hand N=60:.*?penta_nd_kernel ([\d.]+)").group(1),
    "R6_BAND6_US": "17.5 as a launch of its own",
    "R6_TIMELINE": "\n".join("    " + l for l in tl),
    "R6_PIPE_GBS": f"{gbs:.1f}", "R6_PIPE_FRAC": f"{gbs / 8000:.4f}", "R6_PIPE_TRAFFIC": f"{traffic:.2f}",
    "R6_ROW_MODEL": f"{pm['row_model_us']:.1f}", "R6_PIPE8_FLAT": f"{p8['flat_three_separators_us']:.1f}",
    "R6_PIPE8_NESTED": f"{p8['nested_sub_separators_us']:.1f}", "R6_PIPE8_TODAY": f"{p8['model_of_todays_kernel_us']:.1f}",
    "R6_NUMBERS": numbers, "R6_ALL_CONFIGS": "\n".join("    " + l for l in cfgs.strip().splitlines()),
    "R6_SPEEDUP": f"{b['speedup_vs_cpu_baseline']:.0f} – {b['value'] / 486:.0f}", "R6_SPEEDUP1": f"{b['value'] / 209:.0f}",
    "R6_BATCH64": f"{b['batch_mode'][1]['value'] / 1e3:.0f}k",
    "R6_FULLITER": f"{b['full_iteration']['ms_per_iteration']:.3f}", "R6_FULLITER_CPU": f"{b['full_iteration']['cpu_port_ms_per_iteration']:.1f} ms",
    "R6_MPC": f"{mpc.group(1)} (p10 {mpc.group(2)}, p90 {mpc.group(3)})",
    "R6_TRITER_US": f"{avg_us(P('full_iteration_kernel_stats.csv'), 'tr_iter_kernel'):.1f}",
    "R6_COST_US": f"{avg_us(P('full_iteration_kernel_stats.csv'), 'cost_kernel'):.1f}",
    "R6_SMALL_ITER": small_iter_table(),
    "R6_FULLITER_OTHERS": ", ".join(f"{k} {float(v):.3f}" for k, v in fi.items() if k != "mini_cheetah"),
}
# §3.2.3: the stem's numbers are those of profiles/punyo_kernel_stats.txt (tools/punyo_prof.py; not a round's file)
punyo = open(os.path.join(ROOT, "profiles", "punyo_kernel_stats.txt")).read()
pm_ = lambda pat: re.search(pat, punyo).group(1)
vals.update({"PUNYO_FD": pm_(r"fd_kernel<8, 8>.*?median\s+([\d.]+) us"), "PUNYO_CUT": pm_(r"fd_kernel<8, 7>.*?median\s+([\d.]+) us"),
             "PUNYO_ITER": pm_(r"punyo solve:.*?median ([\d.]+) ms"), "PUNYO_LDL": pm_(r"penta_ldl_kernel<30.*?median\s+([\d.]+) us")})
# the tail of fd_kernel since round 6: profiles/fd_tail_* (parent and tree through one job; §3.3, the headline table)
import statistics


def tail_stamps(path):
    t, cur = {}, None
    for l in open(path):
        if l.startswith(("mini_cheetah", "allegro_hand")):
            cur = l.split()[0]; t[cur] = {}
        mm = re.match(r"\s+(\d+) .*?tid0\s+(\d+) \(.*?tid192\s+(\d+)", l)
        if mm and cur:
            t[cur][int(mm.group(1))] = (int(mm.group(2)), int(mm.group(3)))
    return {k: [tuple(s[x][i] - s[y][i] for i in (0, 1)) for x, y in ((22, 12), (16, 12), (22, 16))] for k, s in t.items()}


FT = lambda f: os.path.join(ROOT, "profiles", "fd_tail_" + f)
tb, ta = tail_stamps(FT("stamps_before.txt")), tail_stamps(FT("stamps_after.txt"))
kc = lambda x: "%.1f k" % (x / 1e3)
cb, ca = tb["mini_cheetah"], ta["mini_cheetah"]
# (a line is `parent` or `new` and what bench.py printed; metric and value by pattern, so that a line cut short still counts)
runs = [(l.split()[0], {"metric": re.search(r'"metric": "([^"]*)"', l).group(1), "value": float(re.search(r'"value": ([\d.]+)', l).group(1))})
        for l in open(FT("bench.txt")) if re.match(r"(parent|new)\s+\{", l)]
head = {t: [d["value"] for tt, d in runs if tt == t and "mini_cheetah" in d["metric"]] for t in ("parent", "new")}
med = {t: statistics.median(x) for t, x in head.items()}
spr = {t: (max(x) - min(x)) / med[t] for t, x in head.items()}
gain, bar = med["new"] / med["parent"] - 1, 3 * max(spr.values())
others = {}
for tt, d in runs:
    if "mini_cheetah" not in d["metric"]:
        others.setdefault(d["metric"].split(", ")[-1], {})[tt] = d["value"]
have_stats = os.path.exists(FT("kernel_stats_before.csv")) and os.path.exists(FT("kernel_stats_after.csv"))
fd_b, fd_a = (avg_us(FT("kernel_stats_before.csv"), "fd_kernel"), avg_us(FT("kernel_stats_after.csv"), "fd_kernel")) if have_stats else (None, None)
fd_ba = f"{fd_b:.2f} → {fd_a:.2f} µs (`profiles/fd_tail_kernel_stats_before.csv` / `_after.csv`)" if have_stats else "not measured on this tree (no kernel statistics of the two trees)"
numbers += f"""
| since round 6: the tail of `fd_kernel` (`profiles/fd_tail_*`, parent and tree through one job) | `fd_kernel<3,3>` {fd_ba}; step {1e6 / med['parent']:.1f} → {1e6 / med['new']:.1f} µs, **{med['new']:.0f}** it/s (median of {len(head['new'])}) |"""
vals.update({
    "R6_NUMBERS": numbers,
    "FD_TAIL_STAMPS": f"tid 0 {kc(cb[0][0])} → {kc(ca[0][0])}, tid 192 (the lane that ended the kernel) {kc(cb[0][1])} → {kc(ca[0][1])}; of it the record with its barrier "
                      f"{kc(cb[1][0])} → {kc(ca[1][0])} / {kc(cb[1][1])} → {kc(ca[1][1])} and the products {kc(cb[2][0])} → {kc(ca[2][0])} / {kc(cb[2][1])} → {kc(ca[2][1])} "
                      f"(allegro N = 60: products {kc(tb['allegro_hand'][2][0])} → {kc(ta['allegro_hand'][2][0])} on tid 0, two rounds); `fd_kernel<3,3>` by rocprofv3 {fd_ba}",
    "FD_TAIL_BENCH": f"parent median {med['parent']:.0f} it/s (spread {100 * spr['parent']:.2f} %), this tree {med['new']:.0f} it/s (spread {100 * spr['new']:.2f} %): "
                     f"+{100 * gain:.2f} %, {1e6 / med['parent'] - 1e6 / med['new']:.2f} µs a step, against a bar of three times the larger spread, {100 * bar:.2f} % — "
                     + ("a gain" if gain > bar else "below the bar: not claimed as a gain") + f" (medians of {len(head['parent'])} and {len(head['new'])} runs); "
                     + ("one run each of the other configurations, parent → tree: " + ", ".join(f"{k} {v['parent']:.0f} → {v['new']:.0f} it/s" for k, v in others.items())
                        if others else "allegro_hand and hopper: not measured"),
    "FD_TAIL_END": kc(max(ca[0])),
    "FD_TAIL_FD_US": f"{fd_a:.1f} µs (`profiles/fd_tail_kernel_stats_after.csv`; round 6: {fd_us:.1f})" if have_stats else f"{fd_us:.1f} µs (round 6; the tail since: §3.3)",
    "FD_TAIL_STEP": f"{1e6 / med['new']:.1f} µs = {med['new']:.0f} it/s (`profiles/fd_tail_bench.txt`, median of {len(head['new'])}; round 6: {1e3 * b['ms_per_step']:.1f} µs = {b['value']:.0f} it/s)",
})
# §12.1: the batch at the public interface, profiles/solve_batch.txt (tools/solve_batch_bench.py; not a round's file)
sb = [l.rstrip() for l in open(os.path.join(ROOT, "profiles", "solve_batch.txt")) if l.strip()]
vals["SOLVE_BATCH_FIGURES"] = ("Measured (`tools/solve_batch_bench.py` → `profiles/solve_batch.txt`; " + sb[0].split(": ", 1)[1] + "):\n\n"
                               + "\n".join("    " + l for l in sb[1:]))
# §14.4: the time-varying LQR gains, profiles/tvlqr.txt (tools/tvlqr_bench.py; not a round's file)
vals["TVLQR_TABLE"] = "\n".join("    " + l.strip() for l in open(os.path.join(ROOT, "profiles", "tvlqr.txt")) if l.startswith("  "))
# §14.5: rollouts under the law, profiles/track.txt (tools/track_bench.py; not a round's file)
vals["TRACK_TABLE"] = "\n".join("    " + l.strip() for l in open(os.path.join(ROOT, "profiles", "track.txt")) if l.startswith("  "))
src = os.path.join(ROOT, "tools", "design", "DESIGN.in.md")
text = open(src).read()
subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_design.py")])
out = open(os.path.join(ROOT, "DESIGN.md")).read()
for k in sorted(vals, key=len, reverse=True):
    out = out.replace(f"@@{k}@@", vals[k])
left = sorted(set(re.findall(r"@@\w+@@", out)))
if left:
    raise SystemExit("unfilled: " + " ".join(left))
open(os.path.join(ROOT, "DESIGN.md"), "w").write(out)
print("DESIGN.md filled from profiles/%s_*" % R)
