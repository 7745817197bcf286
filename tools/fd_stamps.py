"""In-kernel clock stamps of fd_kernel (a library built with -DIDTO_FD_STAMPS: tools/fd_variants.sh stamps "-DIDTO_FD_STAMPS";
run with IDTO_HIP_LIB=build/variants/stamps/libidto_hip.so).  Block k = 1, lanes tid 0 (the record's own evaluation,
path 0) and tid 192 (a mass-matrix column; a helper lane of the lane map without the redundant path lanes): shader-clock
cycles since the block's start.  A library built with -DIDTO_FD_STAMP_TID=<tid> stamps that lane in the place of tid 192
(IDTO_FD_STAMP_TID=<tid> in the environment names it here): 100 is a single-path main lane of wavefront 1, 128 a helper with a
pair of the last slot.  Behind the table every stamp of both lanes is listed on tid 0's clock: a lane's clock starts when
its wavefront does, and the release of the evaluation barrier (stamp 12) is one instant for the whole block."""
import os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
NAMES = ["start", "loads issued", "barrier 1", "v/a/edq + barrier 2 + outputs issued", "eval: inputs in registers", "eval: sincos",
         "eval: common body + its pairs", "eval: slot 0 done", "eval: last slot kinematics", "eval: last slot pairs",
         "eval: trailing pairs", "eval: backward pass", "evaluations + barrier", "record: reads landed", "record: divisions done",
         "record: stores issued", "barrier", "products: last tile decoded", "products: last tile, operand step 0",
         "products: last tile, all operand steps", "products: last tile stored", "products: tiles done", "g rows + end",
         # (the lane map without the redundant path lanes, option fd_dedup - IDTO_FD_DEDUP=0 in the environment for the other map;
         # out of sequence: 23 lies between 8 and 9, 24 behind 11, and 25 is the helper lane's, tid 192, between the main lanes' 23 and 9)
         "lane map: last slot's state handed over + barrier", "lane map: baseline's sums published + barrier",
         "lane map (helper): the pairs with the world done",
         # (26 lies between 23 and 9, 27 between 24 and 12; 29 and 28 are the helper's, in this order, behind the main lanes' 23 -
         # 28 is taken by a helper that has a pair of the last slot to evaluate: tid 128 has one, tid 192 has none and waits for
         # its wavefront's lanes that have)
         "lane map: own body-foot pair done (before its barrier)", "lane map: single-path lane's sums and copies done",
         "lane map (helper): last slot's state in registers", "lane map (helper): hand-over barrier released"]
TID = int(os.environ.get("IDTO_FD_STAMP_TID", "192"))   # the second stamping lane the library was built with (-DIDTO_FD_STAMP_TID=...)
NS = int(re.search(r"#define IDTO_FD_NSTAMPS (\d+)", open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "idto_amd", "csrc", "id_fast.h")).read()).group(1))   # slots per stamping lane
for name, N in ((sys.argv[1], int(sys.argv[2])),) if len(sys.argv) > 2 else (("mini_cheetah", 40), ("allegro_hand", 60)):
    cfg = load_config(name); model = load_model(name)
    if 2 * NS > model.nq * model.nv:   # (the kernel returns the stamps in N+_2 and writes none where they do not fit: acrobot, hopper, spinner)
        raise SystemExit(f"{name}: nq * nv = {model.nq * model.nv} doubles of N+_2 cannot hold 2 x {NS} stamps")
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
    dev = hip.HipPath(model, prob, sp); dev.set_q(q)
    acc = np.zeros(2 * NS); n = 0
    for it in range(30):
        dev.eval_partials(); dev.sync()
        v = np.zeros(dev.array_size("nplus")); hip._chk(hip.lib().idto_hip_get(dev.h, hip.ARR["nplus"], hip.dptr(v))); v = v[2 * model.nq * model.nv:][:2 * NS]
        if it >= 10: acc += v; n += 1
    acc /= n
    print(name, "N =", N, "(cycles since the block's start; 100 MHz ticks if the counter is the constant one)")
    for i, nm in enumerate(NAMES):
        if min(acc[i], acc[NS + i]) < 0:   # (a slot the lane did not take holds 0: minus the block's start here)
            col = lambda x: f"{x:9.0f}" if x >= 0 else "        -"
            print(f"  {i:2d} {nm:42s} tid0 {col(acc[i])}              tidB {col(acc[NS+i])}")
            continue
        print(f"  {i:2d} {nm:42s} tid0 {acc[i]:9.0f} (+{acc[i] - (acc[i-1] if i else 0):7.0f})   tidB {acc[NS+i]:9.0f} (+{acc[NS+i] - (acc[NS+i-1] if i else 0):7.0f})")
    # every lane on tid 0's clock: the release of the evaluation barrier (stamp 12) is one instant for the whole block
    off = acc[12] - acc[NS + 12]
    print(f"  on tid 0's clock, aligned at stamp 12 (tidB = tid {TID}: its cycles + {off:.0f}), in order of time:")
    rows = [(acc[i], 0, i) for i in range(NS) if acc[i] >= 0] + [(acc[NS + i] + off, TID, i) for i in range(NS) if acc[NS + i] >= 0 and i != 0]
    for t, lane, i in sorted(rows):
        print(f"    {t:9.0f}  tid {lane:3d}  {i:2d} {NAMES[i]}")
    dev.close()
