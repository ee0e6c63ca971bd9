#!/usr/bin/env python
"""Two builds of the library, same forwards: are the launches, their costs and the results the same, and the times?

    python tools/dispatch_compare.py --parent-lib PATH/libsketchedit_hip.so [--out profiles/NAME.json] [--no-times] [--alternations N]

Each build is selected through SKETCHEDIT_HIP_LIB in a fresh child process (this script with --child).  A child runs
Engine.inference on the same synthetic weights and inputs at 64x64, 40x72 and 256x256, B = 1 and 3, in default, low-latency,
conservative, bf16 and bf16 low-latency mode, with the in-library profiler on, and reports per case the `launches` records of
se_profile_report (form, kernel, layer, workgroups), the per-kernel and per-layer flops / executed flops / bytes, and a SHA-256
of every output tensor's bytes (all finite: equal digests are torch.equal).  Times: the low-latency 256x256 B = 1 call (78
launches in about 1.2 ms: where host time per launch would show; median of five rounds of 200 calls) and bench.py's default
configuration (50 steps, 5 warm-up), N alternations parent / candidate (default 3).  The candidate is within when the median of
its N times exceeds the median of the parent's N by no more than the parent's own spread (max - min of its N).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(64, 64), (40, 72), (256, 256)]
MODES = ["default", "lowlat", "conservative", "bf16", "bf16-lowlat"]
FLAGS = 1 | 2 | 16


def child(out_path, times):
    import torch
    from sketchedit_amd import synth
    from sketchedit_amd._lib import Engine
    eng = Engine(0)
    eng.load_state_dict("M", synth.make_state_dict("M", 0))
    eng.load_state_dict("G", synth.make_state_dict("G", 0))
    cases = {}
    for H, W in SIZES:
        for B in (1, 3):
            img, sk = synth.make_inputs(B, H, W, seed=1234)
            ci, cs = torch.from_numpy(img).cuda(), torch.from_numpy(sk).cuda()
            for mode in MODES:
                eng.set_precision("bf16" if mode.startswith("bf16") else "f32")
                eng.set_conservative(mode == "conservative")
                eng.profile(True)
                try:
                    r = eng.inference(ci, cs, FLAGS, low_latency="lowlat" in mode)
                    torch.cuda.synchronize()
                    rep = eng.profile_report()
                finally:
                    eng.profile(False)
                for sec in ("kernels", "layers"):
                    for rec in rep[sec]:
                        rec.pop("total_ms")
                outs = {}
                for k in sorted(r):
                    t = r[k].detach().float().cpu().contiguous()
                    assert torch.isfinite(t).all(), (H, W, B, mode, k)
                    outs[k] = hashlib.sha256(t.numpy().tobytes()).hexdigest()
                cases["%dx%d B=%d %s" % (H, W, B, mode)] = {"report": rep, "outputs": outs}
    res = {"cases": cases}
    if times:
        eng.set_precision("f32")
        eng.set_conservative(False)
        img, sk = synth.make_inputs(1, 256, 256, seed=1234)
        ci, cs = torch.from_numpy(img).cuda(), torch.from_numpy(sk).cuda()
        for _ in range(50):
            eng.inference(ci, cs, FLAGS, low_latency=True)
        torch.cuda.synchronize()
        rounds = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(200):
                eng.inference(ci, cs, FLAGS, low_latency=True)
            torch.cuda.synchronize()
            rounds.append(1e3 * (time.perf_counter() - t0) / 200)
        res["lowlat_256_b1_ms_rounds"] = [round(v, 4) for v in rounds]
        res["lowlat_256_b1_ms"] = round(sorted(rounds)[2], 4)
    eng.close()
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_child(lib, tag, times, tmp):
    out = os.path.join(tmp, tag + ".json")
    env = dict(os.environ)
    if lib:
        env["SKETCHEDIT_HIP_LIB"] = lib
    else:
        env.pop("SKETCHEDIT_HIP_LIB", None)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out] + ([] if times else ["--no-times"]), env=env, check=True, timeout=400)
    with open(out) as f:
        return json.load(f)


def run_bench(lib, steps, warmup):
    env = dict(os.environ)
    if lib:
        env["SKETCHEDIT_HIP_LIB"] = lib
    else:
        env.pop("SKETCHEDIT_HIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                        "--no-parity", "--no-traffic", "--no-secondary"], env=env, check=True, timeout=400, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    j = json.loads(line)
    return {"ms_per_step": j.get("ms_per_step"), "value": j.get("value")}


def within(parent, cand):
    """median(candidate) - median(parent) <= the parent's own spread between its alternations"""
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return med(cand) - med(parent) <= max(parent) - min(parent)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    ap.add_argument("--no-times", action="store_true")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--alternations", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return child(a.child, not a.no_times)
    alts = "abcdefghijklmnop"[:a.alternations]
    order = [(who + "_" + x, a.parent_lib if who == "parent" else None) for x in alts for who in ("parent", "candidate")]
    runs = {tag: run_child(lib, tag, not a.no_times, a.tmp) for tag, lib in order}
    ref = runs["parent_a"]["cases"]
    diffs = []
    for tag, _ in order[1:]:
        for name, case in runs[tag]["cases"].items():
            if case["report"] != ref[name]["report"]:
                diffs.append("%s: %s: report" % (tag, name))
            if case["outputs"] != ref[name]["outputs"]:
                diffs.append("%s: %s: outputs" % (tag, name))
    res = {"protocol": __doc__.split("\n\n", 2)[2].replace("\n", " ").strip(),
           "cases": len(ref), "launch_records": sum(len(c["report"]["launches"]) for c in ref.values()),
           "reports_identical": not any(d.endswith("report") for d in diffs), "outputs_identical": not any(d.endswith("outputs") for d in diffs),
           "differences": diffs,
           "launches": {name: ["%s:%s:%s:%d" % (r["form"], r["kernel"], r["layer"], r["workgroups"]) for r in c["report"]["launches"]]
                        for name, c in ref.items() if name.endswith("B=1 default") or name.startswith("64x64 B=1")}}
    if not a.no_times:
        ll = {tag: runs[tag]["lowlat_256_b1_ms"] for tag, _ in order}
        bench = {tag: run_bench(lib, 50, 5) for tag, lib in order}
        res["lowlat_256x256_b1_ms"] = ll
        res["lowlat_256x256_b1_ms_rounds"] = {tag: runs[tag]["lowlat_256_b1_ms_rounds"] for tag, _ in order}
        split = lambda d: ([d["parent_" + x] for x in alts], [d["candidate_" + x] for x in alts])      # noqa: E731
        res["lowlat_within_parent_spread"] = within(*split(ll))
        res["bench_default"] = bench
        res["bench_within_parent_spread"] = within(*split({tag: b["ms_per_step"] for tag, b in bench.items()}))
    s = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("launches", "protocol")}))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
