"""Shared by tests/test_id_eval_host.py and tests/test_plant_body_host.py: how the stand-alone host programs over
tests/cpp/lane_emu (the device headers compiled by g++, a lane an OS thread) are built and run, how their case files are
written, and how a thread-sanitizer log is read.  Test infrastructure; no GPU, nothing loaded into Python."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
ASAN = "address,undefined"
TSAN = "thread"


def build(program, out_dir, sanitizer=ASAN):
    """g++ on tests/cpp/<program>.cc with the shim's directory in front of the include path -> the executable"""
    exe = os.path.join(str(out_dir), program + "_" + sanitizer.split(",")[0])
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes",
           "-fsanitize=" + sanitizer]
    if "undefined" in sanitizer:
        cmd.append("-fno-sanitize-recover=undefined")
    cmd += ["-I" + os.path.join(CPP, "lane_emu"), "-I" + CPP, "-I" + os.path.join(ROOT, "idto_amd", "csrc"),
            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), os.path.join(CPP, program + ".cc"),
            os.path.join(ROOT, "idto_amd", "csrc", "host", "model_tables.cc"), "-pthread", "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-6000:]
    return exe


def tsan_unavailable(out_dir):
    """None, or why this toolchain cannot link or start a thread-sanitized program (a probe: an empty main)"""
    src = os.path.join(str(out_dir), "tsan_probe.cc")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    done = subprocess.run(["g++", "-fsanitize=thread", src, "-pthread", "-o", os.path.join(str(out_dir), "tsan_probe")],
                          capture_output=True, text=True)
    if done.returncode != 0:
        return "g++ -fsanitize=thread does not link here: " + done.stderr.strip()[-300:]
    ran = subprocess.run([os.path.join(str(out_dir), "tsan_probe")], capture_output=True, text=True)   # (the runtime maps its shadow at start-up)
    return None if ran.returncode == 0 else "a thread-sanitized empty main does not start here: " + ran.stderr.strip()[-300:]


def fmt(values):
    return " ".join(repr(float(x)) for x in np.ravel(values))


def save_model(model, out_dir, name):
    path = os.path.join(str(out_dir), name + ".model")
    model.save(path)
    return path


def contact_values(sp):
    return [sp.contact_stiffness, sp.dissipation_velocity, sp.stiction_velocity, sp.friction_coefficient, sp.smoothing_factor]


def run(exe, args):
    """-> (return code, the lines of stdout, stderr)"""
    done = subprocess.run([exe] + list(args), capture_output=True, text=True)
    return done.returncode, done.stdout.strip().split("\n"), done.stderr


ACCESS = re.compile(r"^\s+(Previous )?(write|read|atomic write|atomic read) of size \d+ at (0x[0-9a-f]+)", re.I | re.M)


def tsan_reports(stderr):
    """the thread sanitizer's reports in a log: [(kind, [(is a plain write, address), ...])]"""
    out = []
    for block in stderr.split("WARNING: ThreadSanitizer: ")[1:]:
        kind = block.split("(pid=")[0].strip()
        out.append((kind, [(m.group(2).lower() == "write", int(m.group(3), 16)) for m in ACCESS.finditer(block)]))
    return out


def unexpected_tsan_reports(stderr, allowed=None):
    """every report but a data race whose two accesses are both writes inside [allowed[0], allowed[1])"""
    bad = []
    for kind, accesses in tsan_reports(stderr):
        ok = (allowed is not None and kind == "data race" and len(accesses) == 2
              and all(w and allowed[0] <= a < allowed[1] for w, a in accesses))
        if not ok:
            bad.append((kind, accesses))
    return bad
