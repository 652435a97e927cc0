"""Crops of tubes and tracks on the device: ``tuber_tube_crops`` called directly and held, byte for byte, to
``crops.crop_rows`` -- the output between 64 guard bytes of 0xA5 on either side that must survive -- at the output sizes, sample counts, frame
ratios and boxes at which the kernel takes another path; the width limit; the table form; every refusal; and ``VideoDetector(...,
keep_video=True)`` with ``crops()`` end to end on the name-hashed AVA model of tests/test_video_gpu.py.  No tolerance appears anywhere."""
import os

import numpy as np
import pytest
import torch

from test_tube_crops_cpu import H, N, W, case_boxes, video
from tubelet_transformer_amd import input_pipeline as ip
from tubelet_transformer_amd import lib, synth
from tubelet_transformer_amd.config import load_cfg
from tubelet_transformer_amd.crops import crop_rows, crop_table, normalized, tube_crops
from tubelet_transformer_amd.detect import ACTOR_FIELDS, FIELDS
from tubelet_transformer_amd.tuber import build_model
from tubelet_transformer_amd.video import VideoDetector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL, EINVAL = 64, 0xA5, -1


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel's operands and its guarded outputs
# ------------------------------------------------------------------------------------------------------------------------------
def guarded(dev, nbytes, front=GUARD):
    """(the whole buffer, its ``nbytes`` in the middle): ``front`` guard bytes before and GUARD behind, everything 0xA5"""
    buf = torch.full((front + nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[front:front + nbytes]


def guards_intact(buf, nbytes, front=GUARD):
    host = buf.cpu().numpy()
    return bool((host[:front] == FILL).all() and (host[front + nbytes:] == FILL).all())


def operands(fr, index, boxes, dev, offset=0):
    """the video at byte offset ``offset`` of its allocation, the table as ``tube_crops`` uploads it"""
    buf = torch.zeros(offset + fr.size, dtype=torch.uint8, device=dev)
    buf[offset:].copy_(torch.from_numpy(fr).reshape(-1))
    return dict(frames=buf[offset:], N=fr.shape[0], H=fr.shape[1], W=fr.shape[2], frame_index=torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(dev),
                boxes=torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(dev), R=len(index))


def args_of(o, size, source_size, scale, samples, lut, out, valid, over=()):
    a = dict(o, h=size[0], w=size[1], fx=float(np.float64(o["W"]) / np.float64(source_size[1])), fy=float(np.float64(o["H"]) / np.float64(source_size[0])),
             scale=scale, samples=samples, lut=lut, out=out, valid=valid)
    a.update(dict(over))
    return tuple(a[k] for k in ("frames", "N", "H", "W", "frame_index", "boxes", "R", "h", "w", "fx", "fy", "scale", "samples", "lut", "out", "valid"))


def device_crops(fr, index, boxes, size, dev, source_size=None, scale=1.0, samples=1, lut=None, front=GUARD, offset=0):
    """``tuber_tube_crops`` into guarded buffers -> (the output's bytes, valid), the guards checked"""
    o = operands(fr, index, boxes, dev, offset)
    nbytes = len(index) * size[0] * size[1] * 3 * (4 if lut is not None else 1)
    buf, out = guarded(dev, nbytes, front)
    vbuf, valid = guarded(dev, len(index))
    lib.call("tuber_tube_crops", *args_of(o, size, source_size or fr.shape[1:3], scale, samples, lut, out, valid))
    assert guards_intact(buf, nbytes, front) and guards_intact(vbuf, len(index))
    return out.cpu().numpy(), valid.cpu().numpy()


def assert_same_pixels(got, want):
    got = got.reshape(want.shape)
    assert np.array_equal(got, want), "%d of %d bytes differ, first at %s" % ((got != want).sum(), want.size, np.argwhere(got != want)[:4].tolist())


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel against the definition
# ------------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (7, 5), (16, 16), (33, 21), (2, 87))      # odd sizes, h * w * 3 no multiple of 4, a line longer than a workgroup
SOURCES = ((H, W), (2 * H, 2 * W), (100, 141))


@pytest.mark.parametrize("samples", (1, 2, 3))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_kernel_writes_the_definitions_bytes(dev, size, samples):
    assert (3 * W) % 4 != 0 and (3 * W) % 16 != 0
    fr = video()
    index, boxes = case_boxes()
    for source_size in SOURCES:
        for scale in (1.0, 1.5):
            want, want_valid = crop_rows(fr, index, boxes, size, source_size=source_size, scale=scale, samples=samples)
            got, valid = device_crops(fr, index, boxes, size, dev, source_size, scale, samples)
            assert np.array_equal(valid, want_valid) and 0 < want_valid.sum() < len(index), (source_size, scale)
            assert_same_pixels(got, want)
    assert want.any() and not want[want_valid == 0].any()


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_an_output_and_a_video_at_any_byte_alignment(dev, offset):
    fr = video()
    index, boxes = case_boxes()
    for size, samples in (((7, 5), 2), ((16, 16), 1), ((2, 87), 1)):
        want, want_valid = crop_rows(fr, index, boxes, size, samples=samples)
        got, valid = device_crops(fr, index, boxes, size, dev, samples=samples, front=GUARD + offset, offset=4 - offset)
        assert np.array_equal(valid, want_valid)
        assert_same_pixels(got, want)


def test_rows_over_many_workgroups(dev):
    rng = np.random.default_rng(5)
    fr = video(2, (9, H, W))
    R = 130
    index = rng.integers(-1, 10, R).astype(np.int32)                     # -1 and 9 among them
    xy = rng.uniform(-8, 50, (R, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(0.5, 30, (R, 2))], axis=1).astype(np.float32)
    boxes[::17, 0] = np.nan
    assert (index == -1).any() and (index == 9).any()
    for samples in (1, 4):
        want, want_valid = crop_rows(fr, index, boxes, (5, 3), samples=samples)
        got, valid = device_crops(fr, index, boxes, (5, 3), dev, samples=samples)
        assert np.array_equal(valid, want_valid) and 0 < want_valid.sum() < R
        assert_same_pixels(got, want)
    tall, tall_valid = crop_rows(fr, index[:9], boxes[:9], (75, 40), samples=2)  # a crop of many bands, the last one short
    got, valid = device_crops(fr, index[:9], boxes[:9], (75, 40), dev, samples=2)
    assert np.array_equal(valid, tall_valid)
    assert_same_pixels(got, tall)


def test_the_width_limit(dev):
    limit = lib.query("tuber_tube_crops_limits", 0)
    fr = video(3, (1, 4, limit))
    assert fr.nbytes == 4 * limit * 3
    index = np.zeros(5, dtype=np.int32)
    boxes = np.asarray([(0, 0, limit, 4), (limit - 40.5, 0.5, limit + 3, 3.5), (-3, 1, 17.25, 3), (limit, 0, 0, 4), (limit / 2 - 9, 1, limit / 2 + 9, 2)], dtype=np.float32)
    for size, samples in (((3, 9), 1), ((2, 5), 4)):
        want, want_valid = crop_rows(fr, index, boxes, size, samples=samples)
        got, valid = device_crops(fr, index, boxes, size, dev, samples=samples)
        assert valid.tolist() == want_valid.tolist() == [1] * 5
        assert_same_pixels(got, want)
    wide = video(3, (1, 4, limit + 1))                                    # one pixel wider: refused, nothing written
    o = operands(wide, index, boxes, dev)
    buf, out = guarded(dev, 5 * 3 * 9 * 3)
    vbuf, valid = guarded(dev, 5)
    assert lib.call_rc("tuber_tube_crops", *args_of(o, (3, 9), wide.shape[1:3], 1.0, 1, None, out, valid)) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and bool((vbuf == FILL).all())


@pytest.mark.parametrize("size", ((7, 5), (16, 16), (2, 87)), ids=lambda s: "%dx%d" % s)
def test_the_table_form(dev, size):
    fr = video()
    index, boxes = case_boxes()
    table = ip.normalize_lut()
    lut = ip._device_tables(dev, (ip.MEAN, ip.STD))[0]
    assert tuple(lut.shape) == (3, 256) and lut.cpu().numpy().tobytes() == table.tobytes()   # the table tuber_video_clips reads
    for samples, source_size in ((1, (H, W)), (2, (100, 141))):
        pixels, want_valid = crop_rows(fr, index, boxes, size, source_size=source_size, samples=samples)
        want = normalized(pixels, table)
        assert want.shape == (len(index), 3) + size and want.dtype == np.float32
        got, valid = device_crops(fr, index, boxes, size, dev, source_size, samples=samples, lut=lut)
        assert np.array_equal(valid, want_valid) and got.tobytes() == want.tobytes()


def test_refusals_write_nothing(dev):
    fr = video()
    index, boxes = case_boxes()
    R, size = len(index), (7, 5)
    o = operands(fr, index, boxes, dev)
    buf, out = guarded(dev, R * 7 * 5 * 3 * 4)                              # room for either form
    vbuf, valid = guarded(dev, R)
    lut = ip._device_tables(dev, (ip.MEAN, ip.STD))[0]
    shifted = torch.zeros(R * 16 + 16, dtype=torch.uint8, device=dev)
    nan, inf = float("nan"), float("inf")
    lim = [lib.query("tuber_tube_crops_limits", k) for k in range(3)]
    assert lim[2] == 4
    bad = [dict(W=lim[0] + 1), dict(h=lim[1] + 1), dict(w=lim[1] + 1), dict(samples=lim[2] + 1),
           dict(h=0), dict(w=0), dict(samples=0), dict(h=-1), dict(w=-2), dict(samples=-1), dict(N=-1), dict(R=-1), dict(H=-1), dict(W=-1)]
    bad += [{k: v} for k in ("fx", "fy", "scale") for v in (0.0, -1.0, nan, inf, -inf)]
    bad += [{k: None} for k in ("frames", "frame_index", "boxes", "out", "valid")]
    bad += [dict(boxes=shifted[4:]), dict(boxes=shifted[8:]), dict(frame_index=shifted[1:]), dict(frame_index=shifted[2:])]
    for over in bad:
        code = lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, None, out, valid, over))
        assert code == EINVAL, (over, code)
    for over in (dict(out=out[1:]), dict(out=out[2:]), dict(lut=lut.view(torch.uint8).reshape(-1)[1:]), dict(out=None), dict(scale=nan), dict(W=lim[0] + 1)):
        code = lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, lut, out, valid, over))
        assert code == EINVAL, (over, code)                                # the fp32 form wants a 4-byte aligned out and table
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and bool((vbuf == FILL).all())
    none = dict(R=0, frames=None, frame_index=None, boxes=None, out=None, valid=None)
    assert lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, None, out, valid, dict(R=0))) == 0
    assert lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, None, out, valid, none)) == 0
    torch.cuda.synchronize()
    assert bool((buf == FILL).all()) and bool((vbuf == FILL).all())
    assert lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, None, out, valid, dict(out=out[1:]))) == 0     # bytes go anywhere
    assert lib.call_rc("tuber_tube_crops", *args_of(o, size, (H, W), 1.0, 1, None, out, valid)) == 0                          # and the call itself is fine
    want, want_valid = crop_rows(fr, index, boxes, size)
    assert_same_pixels(out[:want.size].cpu().numpy(), want)
    assert np.array_equal(valid.cpu().numpy(), want_valid) and guards_intact(buf, R * 7 * 5 * 3 * 4) and guards_intact(vbuf, R)


def test_tube_crops_on_device_frames(dev, capsys):
    fr = video(1, (60, H, W))
    tubes = [dict(frames=list(range(3, 40)), boxes=np.linspace((2, 3, 20, 30), (25.5, 1.25, 60, 41), 37).astype(np.float32)),
             dict(frames=[], boxes=np.zeros((0, 4), np.float32)), dict(frames=[59, 60, 0], boxes=np.asarray([(0, 0, W, H)] * 3, np.float32))]
    index, boxes, offsets = crop_table(tubes)
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        got = tube_crops(torch.from_numpy(fr).to(dev), tubes, (12, 9), source_size=(2 * H, 2 * W), scale=1.25, samples=2)
        table = tube_crops(torch.from_numpy(fr).to(dev), tubes, (12, 9), normalize=True)
        none = tube_crops(torch.from_numpy(fr).to(dev), [], (12, 9))
    finally:
        lib.set_launch_hook(None)
    assert seen == ["tuber_tube_crops"] * 2 and got.path == table.path == none.path == "device" and capsys.readouterr().err == ""
    want, want_valid = crop_rows(fr, index, boxes, (12, 9), source_size=(2 * H, 2 * W), scale=1.25, samples=2)
    pixels, valid = got.to_host()
    assert got.pixels.is_cuda and np.array_equal(pixels, want) and valid.tolist() == want_valid.tolist() == [1] * 38 + [0, 1]
    assert [tuple(got[i].shape) for i in range(3)] == [(37, 12, 9, 3), (0, 12, 9, 3), (3, 12, 9, 3)] and len(got) == 3 and len(none) == 0
    assert np.array_equal(got[2].cpu().numpy(), want[37:])
    assert table.pixels.cpu().numpy().tobytes() == normalized(crop_rows(fr, index, boxes, (12, 9))[0], ip.normalize_lut()).tobytes()
    big = lib.query("tuber_tube_crops_limits", 1) + 1                       # beyond the kernel's bounds: the definition, and a line that says so
    host = tube_crops(torch.from_numpy(fr).to(dev), tubes[2:], (1, big))
    err = capsys.readouterr().err
    assert host.path == "host" and err.count("\n") == 1 and "beyond" in err and host.pixels.is_cuda
    assert np.array_equal(host.pixels.cpu().numpy(), crop_rows(fr, index[37:], boxes[37:], (1, big))[0])


# ------------------------------------------------------------------------------------------------------------------------------
# VideoDetector(..., keep_video=True) end to end
# ------------------------------------------------------------------------------------------------------------------------------
SIZE = 48                                                                # working resolution 48 x 80, as tests/test_video_gpu.py


def _model(name):
    cfg = load_cfg(os.path.join(ROOT, "configuration", name))
    cfg.CONFIG.DATA.IMG_SIZE = SIZE
    model, _, _ = build_model(cfg)
    synth.load_name_hashed(model)
    model.to(torch.device("cuda:0")).eval()
    return cfg, model


def _hooked(fn):
    seen = []
    lib.set_launch_hook(lambda name, args, launch: (seen.append(name), launch(name, *args))[1])
    try:
        return fn(), seen
    finally:
        lib.set_launch_hook(None)


def test_video_detector_keeps_the_video_and_crops_tubes_and_tracks(dev, capsys):
    cfg, model = _model("TubeR_CSN50_AVA21.yaml")
    kw = dict(actor_thr=0.0, score_thr=0.0, topk=8, actors=8, graphed=False)
    frames = np.random.default_rng(11).integers(0, 256, (64, 96, 160, 3), dtype=np.uint8)
    vd = VideoDetector(cfg, model, batch=2, keep_video=True, **kw)(frames, stride=9)
    assert vd.source_size == (96, 160) and tuple(vd.video.shape) == (64, 48, 80, 3) and vd.video.dtype == torch.uint8 and vd.video.is_cuda
    video_host = vd.video.cpu().numpy()
    for name, tubes in (("tubes", vd.tubes(dense=True)), ("tracks", vd.actors.tracks(dense=True))):
        assert len(tubes) >= 1 and sum(len(t["frames"]) for t in tubes) >= 8, name
        got, seen = _hooked(lambda: vd.crops(tubes, size=(16, 12)))
        assert seen == ["tuber_tube_crops"] and got.path == "device", name
        index, boxes, offsets = crop_table(tubes)
        want, want_valid = crop_rows(video_host, index, boxes, (16, 12), source_size=vd.source_size)
        pixels, valid = got.to_host()
        assert np.array_equal(valid, want_valid) and valid.all() and np.array_equal(got.offsets, offsets) and len(got) == len(tubes)
        assert_same_pixels(pixels, want)
        assert tuple(got[0].shape) == (len(tubes[0]["frames"]), 16, 12, 3) and len(np.unique(want)) > 16
    dflt = vd.crops(vd.tubes()[:1], samples=2, normalize=True)              # CONFIG.VAL.CROPS' size; the key frames only
    assert tuple(dflt.pixels.shape[1:]) == (3, 112, 112) and dflt.pixels.dtype == torch.float32 and dflt.path == "device"
    plain = VideoDetector(cfg, model, batch=2, **kw)(frames, stride=9)
    assert plain.video is None and plain.source_size is None and plain.keys == vd.keys
    for k in FIELDS:
        assert torch.equal(getattr(plain, k), getattr(vd, k)), k
    for k in ACTOR_FIELDS:
        assert torch.equal(getattr(plain.actors, k), getattr(vd.actors, k)), k
    with pytest.raises(RuntimeError, match="keep_video=True"):
        plain.crops(plain.tubes())
    assert "on the host" not in capsys.readouterr().err
