"""Demo-path probe: the per-request wall time of serve.process_image (demo.py:39-73) with the host steps (Pillow + torch
around the forward, device_io=False) and with the steps on the device (device_io=True), B=1, in both execution modes, at
641x481, 1283x963 and 1921x1081; plus the resize kernels' times and effective bandwidth (the bytes each pass must move:
input read once, output written once) from se_profile_report over one device-path request.  Prints one JSON line.

    python tools/serve_probe.py [--reps N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((641, 481), (1283, 963), (1921, 1081))
ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")


def make_model(out_dir):
    import torch
    from sketchedit_amd import models, synth
    from sketchedit_amd.options.test_options import TestOptions
    opt = TestOptions().parse(ARGV.format(d=out_dir).split(), quiet=True)
    opt.isSkip = True
    m = models.create_model(opt)
    m.netG.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("G", 0).items()})
    m.netM.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("M", 0).items()})
    return m.eval()


def wall_ms(fn, reps):
    fn()
    fn()                                   # warm-up: plans, workspace, coefficient tables, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                               # ends in a device-to-host copy: the request is complete
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tempfile
    import numpy as np
    import torch
    from PIL import Image
    from sketchedit_amd import serve
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    model = make_model(tempfile.mkdtemp())
    eng = model.engine()
    rng = np.random.RandomState(0)
    cases = []
    for w, h in SIZES:
        img = Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        sk = Image.fromarray(((rng.rand(h, w) < 0.01) * 255).astype(np.uint8))
        case = dict(w=w, h=h, working=[w // 8 * 8, h // 8 * 8])
        for ll in (True, False):
            tag = "low_latency" if ll else "default"
            host = wall_ms(lambda: serve.process_image(model, img, sk, low_latency=ll), args.reps)
            dev = wall_ms(lambda: serve.process_image(model, img, sk, low_latency=ll, device_io=True), args.reps)
            same = np.array_equal(np.asarray(serve.process_image(model, img, sk, low_latency=ll)),
                                  np.asarray(serve.process_image(model, img, sk, low_latency=ll, device_io=True)))
            case[tag] = dict(host_ms=host, device_io_ms=dev, speedup=round(host["median"] / dev["median"], 2), identical=same)
        eng.profile(True)
        serve.process_image(model, img, sk, device_io=True)
        rep = eng.profile_report()
        eng.profile(False)
        for k in rep["kernels"]:
            if k["kernel"] in ("resize_h", "resize_v"):
                case[k["kernel"]] = dict(launches=k["launches"], ms=round(k["total_ms"], 4), bytes=int(k["bytes"]),
                                         gbps=round(k["bytes"] / (k["total_ms"] * 1e-3) / 1e9, 1) if k["total_ms"] else None)
        cases.append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
    res = dict(tool="serve_probe", B=1, reps=args.reps, torch_threads=torch.get_num_threads(), hbm_peak_gbps_measured=6290,
               cases=cases)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
