"""GPU tests of the demo's per-request steps on the device (demo.py:39-73, process_image): the Pillow-exact resize
kernels (se_resize_u8), the fused input preparation (se_prepare_u8), the whole request as one call (se_edit_u8) and the
serving paths built on them (serve.process_image / BatchingServer with device_io=True).  Every comparison is exact: the
device path must give the bytes the host path (Pillow + torch) gives."""
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resample_util as R
from sketchedit_amd import _lib, serve, synth

pytestmark = pytest.mark.gpu

ARGV = ("--batchSize 1 --name celeb --joint_train_inp --dataset_mode testimage --image_dirs x --mask_dirs x "
        "--image_lists x --model editline2 --netG deepfillc2 --pool_type max --use_cam --output_dir {d} --gpu_ids 0")
FILTERS = [R.BICUBIC, R.BILINEAR, R.LANCZOS]
SWEEP = [((70, 67), (70, 67)), ((70, 67), (70, 64)), ((70, 67), (64, 67)), ((641, 481), (640, 480)), ((70, 67), (64, 64)),
         ((320, 160), (64, 32)), ((40, 24), (120, 72)), ((1, 9), (5, 1)), ((7, 1), (1, 3)), ((999, 5), (16, 16)),
         ((300, 17), (37, 160)), ((33, 33), (33, 40)), ((68, 30), (68, 41))]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from sketchedit_amd import models
    from sketchedit_amd.options.test_options import TestOptions
    opt = TestOptions().parse(ARGV.format(d=tmp_path_factory.mktemp("out")).split(), quiet=True)
    opt.isSkip = True                      # no checkpoint on disk: procedural weights
    m = models.create_model(opt)
    m.netG.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("G", 0).items()})
    m.netM.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict("M", 0).items()})
    return m.eval()


def _request(rng, w, h, sk_size=None, sk_mode="L"):
    img = Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
    sw, sh = sk_size or (w, h)
    lines = ((rng.rand(sh, sw) < 0.01) * 255).astype(np.uint8)
    sk = Image.fromarray(lines)
    if sk_mode == "RGB":
        sk = Image.fromarray(np.stack([lines, rng.randint(0, 256, (sh, sw), dtype=np.uint8), lines // 2], -1))
    elif sk_mode != "L":
        sk = sk.convert(sk_mode)
    return img, sk


def _pil(a, filt, size):
    return np.stack([np.asarray(Image.fromarray(x).resize(size, filt)) for x in a])


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("C", [1, 3])
def test_resize_u8_is_pillow(model, filt, C):
    eng = model.engine()
    rng = np.random.RandomState(10 * filt + C)
    for (wi, hi), (wo, ho) in SWEEP:
        B = 3 if (wi, hi) == (70, 67) else 1
        a = rng.randint(0, 256, (B, hi, wi, C) if C == 3 else (B, hi, wi)).astype(np.uint8)
        got = eng.resize_u8(torch.from_numpy(a).cuda(), (ho, wo), filt).cpu().numpy()
        assert np.array_equal(got, _pil(a, filt, (wo, ho))), ((wi, hi), (wo, ho), B)


def test_resize_u8_large_and_unaligned(model):
    """A photo-sized identity (a copy), the 1080p flooring of the demo, and inputs / outputs that are slices of a batch
    (addresses not 16- or 4-byte aligned: the narrower load paths)."""
    eng = model.engine()
    rng = np.random.RandomState(4)
    a = rng.randint(0, 256, (1, 3024, 4032, 3)).astype(np.uint8)
    t = torch.from_numpy(a).cuda()
    out = eng.resize_u8(t, (3024, 4032))
    assert out.data_ptr() != t.data_ptr() and torch.equal(out, t)
    a = rng.randint(0, 256, (2, 1081, 1921, 3)).astype(np.uint8)
    assert np.array_equal(eng.resize_u8(torch.from_numpy(a).cuda(), (1080, 1920)).cpu().numpy(), _pil(a, R.BICUBIC, (1920, 1080)))
    a = rng.randint(0, 256, (3, 67, 70, 3)).astype(np.uint8)
    t = torch.from_numpy(a).cuda()[1:]                        # starts 14070 bytes into the allocation
    for size in ((60, 70), (64, 64), (67, 33)):
        got = eng.resize_u8(t, size).cpu().numpy()
        assert np.array_equal(got, _pil(a[1:], R.BICUBIC, size[::-1])), size
        dst = torch.zeros((3, size[0], size[1], 3), dtype=torch.uint8, device="cuda")
        eng.resize_u8(t, size, out=dst[1:])                  # an output slice
        assert np.array_equal(dst[1:].cpu().numpy(), got) and not dst[0].any(), size


def test_resize_u8_on_two_streams(model):
    """The ctx's intermediate and tables are used in one stream order: a resize on another stream waits for the previous one."""
    eng = model.engine()
    rng = np.random.RandomState(6)
    a = rng.randint(0, 256, (4, 481, 641, 3)).astype(np.uint8)
    b = rng.randint(0, 256, (4, 300, 500, 3)).astype(np.uint8)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        oa = eng.resize_u8(ta, (480, 640))
    with torch.cuda.stream(s2):
        ob = eng.resize_u8(tb, (320, 512))
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), _pil(a, R.BICUBIC, (640, 480)))
    assert np.array_equal(ob.cpu().numpy(), _pil(b, R.BICUBIC, (512, 320)))


@pytest.mark.parametrize("case", [((70, 67), None, "L"), ((641, 481), (300, 200), "L"), ((640, 480), None, "RGB"),
                                  ((83, 70), (90, 61), "RGB"), ((1921, 1081), None, "L")])
def test_prepare_u8_is_to_tensors(model, case):
    """se_prepare_u8 == serve._to_tensors bit for bit (fp32 torch.equal), written into a slot of a batch."""
    (w, h), sk_size, sk_mode = case
    img, sk = _request(np.random.RandomState(w), w, h, sk_size, sk_mode)
    x, m, _ = serve._to_tensors(img, sk)
    H, W = x.shape[2:]
    a, s = serve._device_inputs(img, sk)
    eng = model.engine()
    image = torch.full((3, 3, H, W), 7.0, device="cuda")
    sketch = torch.full((3, 1, H, W), 7.0, device="cuda")
    eng.prepare_u8(_lib.upload_u8(a, "cuda"), _lib.upload_u8(s, "cuda"), H, W, out=(image[1:2], sketch[1:2]))
    assert torch.equal(image[1:2].cpu(), x) and torch.equal(sketch[1:2].cpu(), m)
    assert bool((image[0] == 7).all()) and bool((image[2] == 7).all()) and bool((sketch[0] == 7).all())
    assert 0 < float(m.sum()) < m.numel()


def test_fused_quantisation_needs_no_clamp(model):
    """demo.py:62 clamps the composite to [-1, 1] before (g+1)/2*255 -> uint8; the device path quantises in the forward's
    last kernel without a clamp.  On real requests the bytes agree: the clamp changes no value."""
    rng = np.random.RandomState(8)
    for w, h in ((70, 67), (641, 481)):
        img, sk = _request(rng, w, h)
        x, m, _ = serve._to_tensors(img, sk)
        data = {"image": x.cuda(), "mask": m.cuda()}
        for ll in (True, False):
            with torch.no_grad():
                g, _ = model(dict(data), mode="inference", low_latency=ll)
            clamped = ((torch.clamp(g, -1, 1) + 1) / 2 * 255).cpu().numpy().astype(np.uint8)[0].transpose(1, 2, 0)
            unclamped = ((g + 1) / 2 * 255).cpu().numpy().astype(np.uint8)[0].transpose(1, 2, 0)
            rgb, _ = model.inference_u8(dict(data), low_latency=ll)
            assert np.array_equal(clamped, unclamped), (w, h, ll)
            assert np.array_equal(rgb[0].cpu().numpy(), clamped), (w, h, ll)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("size", [(70, 67), (641, 481), (640, 480), (1921, 1081)])
def test_process_image_device_io_is_the_host_path(model, size):
    w, h = size
    img, sk = _request(np.random.RandomState(w + h), w, h)
    for ll in (True, False):
        host = serve.process_image(model, img, sk, low_latency=ll)
        dev = serve.process_image(model, img, sk, low_latency=ll, device_io=True)
        assert dev.size == img.size and dev.mode == "RGB"
        assert np.array_equal(np.asarray(dev), np.asarray(host)), (size, ll)


def test_edit_u8_batch_and_refusals(model):
    """edit_u8 over B requests of one raw size == each request alone; working sizes under 16 raise (the C-ABI through
    se_last_error, process_image as the host path does); sketch modes the device path does not take use the host path."""
    rng = np.random.RandomState(9)
    reqs = [_request(rng, 75, 66, (60, 50)) for _ in range(3)]
    arrays = [serve._device_inputs(i, s) for i, s in reqs]
    batch = model.edit_u8(np.stack([a for a, _ in arrays]), np.stack([s for _, s in arrays]), low_latency=True)
    for k, (img, sk) in enumerate(reqs):
        one = serve.process_image(model, img, sk, low_latency=True)
        assert np.array_equal(batch[k].cpu().numpy(), np.asarray(one)), k
    with pytest.raises(_lib.SketchEditHipError, match="too small"):
        model.edit_u8(np.zeros((40, 15, 3), np.uint8), np.zeros((40, 15), np.uint8))
    with pytest.raises(ValueError):
        serve.process_image(model, Image.new("RGB", (12, 40)), Image.new("L", (12, 40)), device_io=True)
    for mode in ("1", "P", "RGBA"):
        img, sk = _request(rng, 70, 67, sk_mode=mode)
        assert sk.mode == mode
        assert np.array_equal(np.asarray(serve.process_image(model, img, sk, device_io=True)),
                              np.asarray(serve.process_image(model, img, sk))), mode


@pytest.mark.timeout(180)
def test_batching_server_device_io(model):
    """Concurrent submitters of mixed raw sizes, two of which share a working size (and one whose sketch mode takes the
    host preparation): byte-identical to one-by-one process_image, and the requests of one working size share a forward."""
    rng = np.random.RandomState(12)
    reqs = [_request(rng, 70, 67), _request(rng, 71, 69, (50, 40)), _request(rng, 96, 64), _request(rng, 70, 67, sk_mode="RGB"),
            _request(rng, 69, 70, sk_mode="1"), _request(rng, 96, 65)]
    single = [serve.process_image(model, i, s) for i, s in reqs]
    srv = serve.BatchingServer(model, max_batch=8, max_wait_s=0.3, device_io=True)
    outs = [None] * len(reqs)

    def worker(i):
        outs[i] = srv.submit(*reqs[i])
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(reqs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    srv.close()
    for k, (a, b) in enumerate(zip(single, outs)):
        assert b.size == reqs[k][0].size and np.array_equal(np.asarray(a), np.asarray(b)), k
    assert sum(srv.batches) == len(reqs) and max(srv.batches) >= 2
