"""Streaming attention probe: B=1 forwards at 1216x1216 (materialised and streaming forced), 1080x1920 and 2048x2048, in
fp32 and bf16.  Prints one JSON line: per case the forward time (HIP events, after warm-up), the attention's time and
the executed TFLOP/s of the two streaming kernels (FLOPs booked from the tile shapes launched, times from
se_profile_report), the workspace bytes; plus the 1216x1216 streaming / materialised attention-time ratio.

    python tools/att_stream_probe.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATT = ("att_prep", "att_score", "att_softmax", "att_boxsum", "att_pv", "att_stream_stats", "att_stream_out")
FLAGS = 1 | 2 | 16


def run_case(eng, lib, H, W, precision, stream, reps):
    import torch
    from sketchedit_amd import synth
    lib.set_option("SE_ATT_STREAM", 1 if stream else 0)
    eng.set_precision(precision)
    img, sk = synth.make_inputs(1, H, W, seed=5)
    ci, cs = torch.from_numpy(img).cuda(), torch.from_numpy(sk).cuda()
    eng.inference(ci, cs, FLAGS)                      # warm-up: plans, workspace, code objects
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        eng.inference(ci, cs, FLAGS)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    eng.profile(True)
    eng.inference(ci, cs, FLAGS)
    rep = eng.profile_report()
    eng.profile(False)
    ks = {k["kernel"]: k for k in rep["kernels"]}
    att_ms = sum(ks[k]["total_ms"] for k in ATT if k in ks)
    prof_total = sum(k["total_ms"] for k in rep["kernels"])
    case = dict(H=H, W=W, B=1, precision=precision, form="streaming" if "att_stream_out" in ks else "materialised",
                forward_ms=round(sorted(ms)[len(ms) // 2], 3), forward_ms_min=round(min(ms), 3),
                attention_ms=round(att_ms, 3), attention_share_of_kernel_time=round(att_ms / prof_total, 4) if prof_total else None,
                workspace_bytes=int(eng.lib.se_workspace_bytes(eng.h, 1, H, W)))
    for k in ("att_stream_stats", "att_stream_out"):
        if k in ks:
            case[k + "_ms"] = round(ks[k]["total_ms"], 3)
            case[k + "_tflops_executed"] = round(ks[k]["flops_executed"] / (ks[k]["total_ms"] * 1e-3) / 1e12, 2)
            case[k + "_workgroups"] = ks[k]["workgroups"]
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sketchedit_amd import _lib, synth
    eng = _lib.Engine(0)
    eng.load_state_dict("M", synth.make_state_dict("M", 0))
    eng.load_state_dict("G", synth.make_state_dict("G", 0))
    cases = []
    try:
        for precision in ("f32", "bf16"):
            for (H, W, stream) in ((1216, 1216, False), (1216, 1216, True), (1080, 1920, False), (2048, 2048, False)):
                cases.append(run_case(eng, _lib, H, W, precision, stream, args.reps))
                print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
    finally:
        _lib.set_option("SE_ATT_STREAM", 0)
        eng.close()
    ratio = {}
    for precision in ("f32", "bf16"):
        m = [c for c in cases if c["precision"] == precision and c["H"] == 1216]
        if len(m) == 2 and m[0]["attention_ms"]:
            ratio[precision] = round(m[1]["attention_ms"] / m[0]["attention_ms"], 3)
    res = dict(tool="att_stream_probe", fp32_mfma_peak_tflops=157.3, cases=cases, ratio_1216_streaming_over_materialised=ratio)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
