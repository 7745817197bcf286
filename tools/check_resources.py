#!/usr/bin/env python3
"""Build-time guard on what the register allocator did to the production kernels (VERDICT r4 "weak" #1 iv).

DESIGN.md section 10: an inlined tail once pushed fd_kernel's SGPR spills from 105 to 146 and the kernel then computed
wrong partials without the tail ever running - the hot kernels sit at the edge of what the allocator handles, and only
the parity tests on a GPU would have noticed.  build.sh compiles with -Rpass-analysis=kernel-resource-usage, keeps the
remarks under build/, and runs this script: a production instantiation with spilled vector registers, more scratch
or more spilled scalar registers than the limits below FAILS THE BUILD (exit 1).  tests/test_build_resources.py runs
the same check on the CPU (hipcc cross-compiles without a GPU).

usage: check_resources.py [--compile] [remarks files ...]     (--compile: produce the remarks first, ~90 s)
"""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMARKS = [os.path.join(ROOT, "build", "fd_launch.remarks"), os.path.join(ROOT, "build", "idto_hip.remarks"),
           os.path.join(ROOT, "build", "plant_launch.remarks"), os.path.join(ROOT, "build", "scene_launch.remarks"),
           os.path.join(ROOT, "build", "lin_launch.remarks"), os.path.join(ROOT, "build", "track_launch.remarks")]

# kernel (demangled, without "idto_dev::" and arguments) -> (max spilled VGPRs, max scratch bytes per lane, max spilled SGPRs)
# Values: what profiles/r05_isa_resources.txt records, the SGPR figure with a margin of 24 (it moves by a few with every
# edit and is harmless up to there; 41 more than today's was the incident).
LIMITS = {
    "fd_kernel<2, 1>": (0, 20, 83 + 24),
    "fd_kernel<3, 2>": (0, 20, 87 + 24),
    "fd_kernel<3, 3>": (0, 20, 105 + 24),
    "fd_kernel<3, 5>": (0, 20, 85 + 24),
    "fd_kernel<4, 4>": (0, 20, 107 + 24),
    # (the free object + seven-body arm of the Jaco examples: one path, so the records' addresses are uniform - more of the
    # kernel's values live in scalar registers, and more of those are spilled to lanes; no vector register is spilled)
    "fd_kernel<8, 6>": (0, 20, 161 + 24),
    # (models with shared pairs: the generic evaluation with the chain states and contact sums in LDS - the generic
    # fd_kernel<8, 0> keeps them in registers and spills 584 vector registers to scratch)
    "fd_kernel<8, 7>": (0, 20, 139 + 24),
    # (models with a stem below the common body: the same evaluation, and every lane walks the stem in a loop - its bodies'
    # records and the blocks of the backward pass are in LDS too, beside the chain bodies')
    "fd_kernel<8, 8>": (0, 20, 132 + 24),
    "penta_pipe_kernel<19, false>": (0, 36, 102 + 24),
    "penta_pipe_kernel<2, false>": (0, 0, 137 + 24),
    "penta_pipe_kernel<3, false>": (0, 0, 106 + 24),
    "penta_pipe_kernel<5, false>": (0, 0, 126 + 24),
    # (the instantiations that also decide on the trial point inside idto_hip_tr_solve: one more role, cost_kernel's work)
    "penta_pipe_kernel<19, true>": (0, 36, 204 + 24),
    "penta_pipe_kernel<5, true>": (0, 0, 209 + 24),
    # (round 6: the solver's workgroup became penta_band_body, shared with gn_small.h - the scalar registers of the inlined
    # body are allocated differently, 22 / 48 more of them spill to lanes; the step is unchanged: 26.9 / 38.0 us before and after)
    "penta_band_kernel<6>": (0, 112, 26 + 24),
    "penta_band_kernel<9>": (0, 112, 26 + 24),
    "penta_band_kernel<12>": (0, 112, 66 + 24),
    "penta_band_kernel<15>": (0, 112, 70 + 24),
    # (round 6, second half: the kernel also carries the trust-region loop's cost and decision - 130 / 137 scalar registers
    # spilled to lanes; the plain step's time is what it was, profiles/r06_all_configs.txt)
    "gn_small_kernel<1, 6, 256, 6, false>": (0, 152, 52 + 24),
    "gn_small_kernel<5, 9, 256, 9, false>": (0, 152, 56 + 24),
    # (the trust-region loop's instantiations: cost and decision behind the records, tr_iter_kernel's part in front - a whole
    # iteration of a small model in one launch -, with the enforced constraint the KKT system's blocks of nq + 1)
    "gn_small_kernel<1, 6, 256, 6, true>": (0, 152, 175 + 24),
    "gn_small_kernel<5, 9, 256, 9, true>": (0, 152, 175 + 24),
    "gn_small_kernel<1, 6, 256, 9, true>": (0, 152, 220 + 24),
    "gn_small_kernel<5, 9, 256, 12, true>": (0, 152, 228 + 24),
    "penta_nd_kernel<23, false>": (0, 0, 585 + 24),
    # ("a guard whose limit equals today's spill count guards nothing".  What it guards is the scratch column:
    # the six registers are spilled to ACCUMULATION registers - v_accvgpr_write / _read, no memory - which a kernel of one
    # wavefront per SIMD has 256 of; the limit that matters, 0 bytes of scratch, holds.  Getting the six back would need the
    # 29-row elimination's multipliers out of registers, i.e. penta_pipe.h's read-back scheme in penta_ldl.h: not done.)
    "penta_nd_kernel<29, false>": (6, 0, 869 + 24),
    "assemble_terms_kernel": (0, 0, 6 + 24),
    # (round 6: four instantiations of the row body - 4, 8, 20, 32 band entries per thread in registers - are inlined into
    # tr_iter_kernel, and the kernel carries the workgroup through the whole iteration: 29 -> 70 scalar registers spilled to lanes)
    # (68 B of private segment are RESERVED since the KKT solution is taken apart in here - a stack object whose accesses were
    # all promoted to registers: the kernel has no scratch instruction, build/isa/main.s)
    "tr_iter_kernel": (0, 68, 73 + 24),
    "cost_kernel": (0, 0, 17 + 24),
    # (the linesearch loop and idto_hip_costs_along, csrc/linesearch.h: no spilled register of either kind today)
    # (fd_body with the mode fixed at tau only, the candidate in blockIdx.y: the shapes' kernels, as for fd_kernel)
    "fd_along_kernel<2, 1>": (0, 0, 12 + 24),
    "fd_along_kernel<3, 2>": (0, 0, 12 + 24),
    "fd_along_kernel<3, 3>": (0, 0, 15 + 24),
    "fd_along_kernel<3, 5>": (0, 0, 14 + 24),
    "fd_along_kernel<4, 4>": (0, 0, 16 + 24),
    "fd_along_kernel<8, 6>": (0, 0, 65 + 24),
    "fd_along_kernel<8, 7>": (0, 0, 76 + 24),
    "fd_along_kernel<8, 8>": (0, 0, 65 + 24),
    # (the same with the problem of a batch in blockIdx.z, csrc/fd_kernel.h: three more strides and the problem's own
    # DevProblem - four scalar registers more are spilled to lanes than in fd_along_kernel, no vector register; the
    # one-path shape <8, 6> reserves fd_kernel's 20 B of private segment)
    "fd_along_batch_kernel<2, 1>": (0, 0, 16 + 24),
    "fd_along_batch_kernel<3, 2>": (0, 0, 16 + 24),
    "fd_along_batch_kernel<3, 3>": (0, 0, 19 + 24),
    "fd_along_batch_kernel<3, 5>": (0, 0, 18 + 24),
    "fd_along_batch_kernel<4, 4>": (0, 0, 20 + 24),
    "fd_along_batch_kernel<8, 6>": (0, 20, 69 + 24),
    "fd_along_batch_kernel<8, 7>": (0, 0, 79 + 24),
    "fd_along_batch_kernel<8, 8>": (0, 0, 69 + 24),
    # (a batch with per-problem models, csrc/fd_kernel.h: fd_kernel's and fd_along_batch_kernel's fd_body with the DevModel and
    # the DevContact read from the problem's parameter record through the constant address space instead of the kernel's
    # arguments - no vector register spilled, fd_kernel's 20 B of private segment; where the model's fields were argument
    # registers they are scalar loads' results now, and up to 49 more scalar registers are spilled to lanes)
    # (forward differences on the lane map without the redundant path lanes, csrc/fd_kernel.h fd_body_impl's DD: main lanes and the
    # helper lanes that evaluate their pairs with the world in one kernel.  Held to the limits of fd_kernel<3, 3> and
    # fd_models_kernel<3, 3>, whose rows - the kernels the option fd_dedup = 0 launches - did not move.)
    "fd_dedup_kernel<3, 3>": (0, 20, 105 + 24),
    "fd_dedup_models_kernel<3, 3>": (0, 20, 109 + 24),
    "fd_models_kernel<2, 1>": (0, 20, 90 + 24),
    "fd_models_kernel<3, 2>": (0, 20, 92 + 24),
    "fd_models_kernel<3, 3>": (0, 20, 109 + 24),
    "fd_models_kernel<3, 5>": (0, 20, 91 + 24),
    "fd_models_kernel<4, 4>": (0, 20, 109 + 24),
    "fd_models_kernel<8, 6>": (0, 0, 176 + 24),
    "fd_models_kernel<8, 7>": (0, 20, 169 + 24),
    "fd_models_kernel<8, 8>": (0, 20, 183 + 24),
    "fd_along_models_kernel<2, 1>": (0, 0, 15 + 24),
    "fd_along_models_kernel<3, 2>": (0, 0, 15 + 24),
    "fd_along_models_kernel<3, 3>": (0, 20, 24 + 24),
    "fd_along_models_kernel<3, 5>": (0, 0, 15 + 24),
    "fd_along_models_kernel<4, 4>": (0, 20, 26 + 24),
    "fd_along_models_kernel<8, 6>": (0, 20, 71 + 24),
    "fd_along_models_kernel<8, 7>": (0, 0, 120 + 24),
    "fd_along_models_kernel<8, 8>": (0, 0, 127 + 24),
    # (the plants' kernel, csrc/plant.h: the GENERIC evaluation id_eval<MAXC> for every model - the tree shapes' straight-line
    # evaluation is not in it.  The figures are of the same kind as the generic fd_kernel<MAXC, 0>'s (24 / 28 / 69 / 564 spilled
    # vector registers in this build: the chain's state in registers over the contact loop): up to MAXC = 3 the spills go to
    # accumulation registers, no scratch; MAXC = 4 and 8 spill to scratch as fd_kernel<4, 0> and fd_kernel<8, 0> do
    # (DESIGN.md section 14.2).  The exchange form keeps the chain in LDS and spills no vector register.  The third template
    # argument, STEM, came with plant_kernel<8, true, true>: the five rows before it are the same code under a longer name.)
    "plant_kernel<2, false, false>": (24, 0, 171 + 24),
    "plant_kernel<3, false, false>": (28, 0, 182 + 24),
    "plant_kernel<4, false, false>": (87, 264, 162 + 24),
    "plant_kernel<8, false, false>": (600, 1412, 201 + 24),
    "plant_kernel<8, true, false>": (0, 0, 147 + 24),
    # (a stem below the common body, id_eval<8, true, true>: the exchange form again - no vector register spilled, no scratch; the
    # stem walk's loop state makes it the instantiation with the most scalar registers spilled to lanes beside <8, false, false>)
    "plant_kernel<8, true, true>": (0, 0, 196 + 24),
    # (the scene report's kernel, csrc/scene_report.h: a lane per body, then per pair, then per DoF, the bodies' records and the
    # pairs' rows in LDS - no vector register spilled, no scratch; <true> reads the problem's DevModel and DevContact from its
    # parameter record, <false> from the kernel's arguments: 10 / 3 scalar registers spilled to lanes)
    "scene_kernel<false>": (0, 0, 3 + 24),
    "scene_kernel<true>": (0, 0, 10 + 24),
    # (the linearisation's and the Riccati recursion's kernels, csrc/plant_lin.h: a lane per column and joint, a lane per entry of
    # a product with the matrices in LDS - no vector register spilled, no scratch; tvlqr_kernel spills 11 scalar registers to lanes)
    "lin_perturb_kernel": (0, 0, 0 + 24),
    "lin_difference_kernel": (0, 0, 0 + 24),
    "tvlqr_kernel": (0, 0, 11 + 24),
    # (the plants under the time-varying LQR law, csrc/plant.h: plant_kernel's body with the law at the start of every control
    # step - six more pointers and six more integers live over the substep loop.  Against plant_kernel's rows: 31 to 87 more
    # scalar registers spilled to lanes; <2> and <8, true, false> spill what plant_kernel spills of vector registers, <3> 4 more
    # (now past the accumulation registers: 68 B of scratch), <4> and <8> 25 / 37 more to 100 B more of scratch, and
    # <8, true, true> spills ONE vector register to 8 B of scratch where plant_kernel spills none.  Recorded)
    "track_kernel<2, false, false>": (24, 0, 202 + 24),
    "track_kernel<3, false, false>": (32, 68, 214 + 24),
    "track_kernel<4, false, false>": (112, 364, 229 + 24),
    "track_kernel<8, false, false>": (637, 1512, 265 + 24),
    "track_kernel<8, true, false>": (0, 0, 214 + 24),
    "track_kernel<8, true, true>": (1, 8, 283 + 24),
    "ls_gather_batch_kernel": (0, 0, 0 + 24),
    "ls_trial_kernel": (0, 0, 0 + 24),
    "ls_cost_kernel": (0, 0, 0 + 24),
    "ls_prepare_kernel": (0, 0, 0 + 24),
    "ls_scan_kernel": (0, 0, 0 + 24),
    "ls_finish_kernel": (0, 0, 0 + 24),
}


def compile_remarks():
    """The six translation units with the remark pass on (device code only, no object files kept)."""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Iinclude", "-Iidto_amd/csrc", "-S",
             "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = [([hipcc] + flags + ["idto_amd/csrc/fd_launch.hip", "-o", "/dev/null"], REMARKS[0]),
            ([hipcc] + flags + ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "idto_amd/csrc/idto_hip.hip", "-o", "/dev/null"], REMARKS[1]),
            ([hipcc] + flags + ["idto_amd/csrc/plant_launch.hip", "-o", "/dev/null"], REMARKS[2]),
            ([hipcc] + flags + ["idto_amd/csrc/scene_launch.hip", "-o", "/dev/null"], REMARKS[3]),
            ([hipcc] + flags + ["idto_amd/csrc/lin_launch.hip", "-o", "/dev/null"], REMARKS[4]),
            ([hipcc] + flags + ["idto_amd/csrc/track_launch.hip", "-o", "/dev/null"], REMARKS[5])]
    procs = [(subprocess.Popen(cmd, cwd=ROOT, stderr=open(out, "w")), out) for cmd, out in jobs]
    for p, out in procs:
        if p.wait() != 0:
            sys.stderr.write(open(out).read()[-4000:])
            raise SystemExit("check_resources: compiling for the remarks failed")


def parse(files):
    rows = {}
    for f in files:
        cur = None
        for line in open(f, errors="replace"):
            m = re.search(r"remark: (?:Function Name: (\S+)|\s*(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+))", line)
            if not m:
                continue
            if m.group(1):
                cur = m.group(1); rows[cur] = {}
            elif cur:
                rows[cur][m.group(2)] = int(m.group(3))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(rows, names):
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\(.*", "", name).replace("idto_dev::", "")
        out[name] = rows[mangled]
    return out


def check(files=None):
    """-> (list of violations, table of what was checked)"""
    res = parse(files or REMARKS)
    bad, table = [], []
    for k, (vs, sc, ss) in LIMITS.items():
        if k not in res:
            bad.append(f"{k}: not in the compiler's remarks (instantiation renamed or removed? update tools/check_resources.py)")
            continue
        d = res[k]
        got = (d.get("VGPRs Spill", 0), d.get("ScratchSize [bytes/lane]", 0), d.get("SGPRs Spill", 0))
        table.append((k, got, (vs, sc, ss)))
        if got[0] > vs: bad.append(f"{k}: {got[0]} spilled VGPRs (limit {vs})")
        if got[1] > sc: bad.append(f"{k}: {got[1]} B of scratch per lane (limit {sc})")
        if got[2] > ss: bad.append(f"{k}: {got[2]} spilled SGPRs (limit {ss})")
    return bad, table


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--compile"]
    if "--compile" in sys.argv[1:]:
        compile_remarks()
    bad, table = check(args or None)
    for k, got, lim in table:
        print(f"{k:32s} spilled VGPRs {got[0]:3d} (<= {lim[0]:3d})  scratch {got[1]:4d} B (<= {lim[1]:4d})  spilled SGPRs {got[2]:3d} (<= {lim[2]:3d})")
    if bad:
        print("RESOURCE CHECK FAILED:\n  " + "\n  ".join(bad))
        sys.exit(1)
    print("resource check passed")
