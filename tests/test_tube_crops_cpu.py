"""Crops of tubes and tracks without a GPU: the numpy definition ``crops.crop_values`` / ``crop_rows`` against the
properties that pin its geometry exactly and against fp64 ``grid_sample``, invalid rows, ``crop_table``, the host path of ``tube_crops``, the
settings, the C ABI's declarations and the signatures.  The shared cases of the GPU test live here as well (``CASES``, ``case_boxes``)."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from test_tube_nms_cpu import padded_actors, padded_detections
from tubelet_transformer_amd import input_pipeline as ip
from tubelet_transformer_amd import lib
from tubelet_transformer_amd.config import crop_settings, get_cfg_defaults, load_cfg
from tubelet_transformer_amd.crops import TubeCrops, crop_rows, crop_table, crop_values, normalized, tube_crops
from tubelet_transformer_amd.video import VideoDetections, VideoDetector, VideoStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 3, 37, 53


def video(seed=0, shape=(N, H, W)):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


def f32(rows):
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def case_boxes(n=N, h=H, w=W):
    """(frame_index, boxes) of the rows every comparison runs: interior and sub-pixel, overhanging each edge, entirely outside on each side, the
    whole frame, no area, flipped, 1e-3 wide, +-1e30, NaN / inf coordinates, frame numbers -1 and n"""
    nan, inf = float("nan"), float("inf")
    rows = [(0, (5.3, 4.1, 30.7, 33.2)), (1, (17.25, 9.5, 21.125, 13.875)),
            (2, (-10, 5, 20, 20)), (0, (40, 20, w + 17, 30)), (1, (10, -7.5, 30, 12)), (2, (12, 25, 33, h + 9.25)),
            (0, (-30, 3, -5, 20)), (1, (w + 5, 3, w + 20, 20)), (2, (4, -40, 30, -2)), (0, (4, h + 2, 30, h + 30)),
            (1, (0, 0, w, h)), (2, (10, 10, 10, 10)), (0, (30.7, 4.1, 5.3, 33.2)), (1, (5.3, 33.2, 30.7, 4.1)),
            (2, (20, 11, 20.001, 30)), (0, (-1e30, -1e30, 1e30, 1e30)), (1, (1e30, 3, -1e30, 9)),
            (2, (nan, 1, 5, 9)), (0, (1, 2, inf, 9)), (1, (1, -inf, 4, 9)), (-1, (1, 2, 30, 20)), (n, (1, 2, 30, 20)), (2, (1, 2, 30, 20))]
    return np.asarray([r[0] for r in rows], dtype=np.int32), f32([r[1] for r in rows])


# ------------------------------------------------------------------------------------------------------------------------------
# the definition's geometry, exactly
# ------------------------------------------------------------------------------------------------------------------------------
def test_a_whole_frame_box_at_frame_size_is_the_frame():
    fr = video()
    val, valid = crop_values(fr, [0, 2], f32([(0, 0, W, H)] * 2), (H, W))
    assert np.array_equal(val, fr[[0, 2]].astype(np.float64)) and valid.tolist() == [1, 1] and val.dtype == np.float64
    pix, _ = crop_rows(fr, [0, 2], f32([(0, 0, W, H)] * 2), (H, W))
    assert pix.dtype == np.uint8 and np.array_equal(pix, fr[[0, 2]])


def test_an_integer_aligned_box_at_its_own_size_is_the_slice():
    fr = video()
    val, _ = crop_values(fr, [1], f32([(4, 6, 24, 20)]), (14, 20))
    assert np.array_equal(val[0], fr[1, 6:20, 4:24].astype(np.float64))


def test_two_samples_at_an_exact_halving_are_the_two_by_two_mean():
    fr = video()[:, :36, :52]
    val, _ = crop_values(fr, [0], f32([(0, 0, 52, 36)]), (18, 26), samples=2)
    assert np.array_equal(val[0], fr[0].astype(np.float64).reshape(18, 2, 26, 2, 3).sum((1, 3)) / 4.0)
    pix, _ = crop_rows(fr, [0], f32([(0, 0, 52, 36)]), (18, 26), samples=2)
    assert np.array_equal(pix[0], np.floor(val[0] + 0.5).astype(np.uint8))             # halves round up
    assert (val[0] - np.floor(val[0]) == 0.5).any()


def test_a_flipped_box_is_the_mirrored_crop():
    fr = video()
    box = (4.5, 6.25, 24.5, 20.25)                                                      # steps of 2.5 and 1.75: every position exact
    val, _ = crop_values(fr, [1, 1, 1], f32([box, (24.5, 6.25, 4.5, 20.25), (4.5, 20.25, 24.5, 6.25)]), (8, 8))
    assert not np.array_equal(val[0], np.floor(val[0]))                                 # fractional weights took part
    assert np.array_equal(val[1], val[0][:, ::-1]) and np.array_equal(val[2], val[0][::-1])


def test_a_box_beyond_an_edge_replicates_the_edge():
    fr = video()
    beyond = f32([(W + 5, 3, W + 20, 20), (-30, 3, -5, 20), (4, H + 2, 30, H + 30), (4, -40, 30, -2)])
    val, valid = crop_values(fr, [1] * 4, beyond, (7, 5))
    assert valid.tolist() == [1] * 4
    for k, col in ((0, W - 1), (1, 0)):                                                 # the last / first column, resampled down the lines only
        want, _ = crop_values(np.ascontiguousarray(fr[:, :, col:col + 1]), [1], f32([(0, 3, 1, 20)]), (7, 1), source_size=(H, 1))
        assert np.array_equal(val[k], np.repeat(want[0], 5, axis=1))
    for k, line in ((2, H - 1), (3, 0)):
        want, _ = crop_values(np.ascontiguousarray(fr[:, line:line + 1]), [1], f32([(4, 0, 30, 1)]), (1, 5), source_size=(1, W))
        assert np.array_equal(val[k], np.repeat(want[0], 7, axis=0))


def test_scale_two_is_the_box_doubled_about_its_centre():
    fr = video()
    val, _ = crop_values(fr, [0, 2], f32([(8, 8, 16, 24), (20.5, 3.25, 30.5, 9.75)]), (9, 7), scale=2.0, samples=2)
    want, _ = crop_values(fr, [0, 2], f32([(4, 0, 20, 32), (15.5, 0, 35.5, 13)]), (9, 7), samples=2)
    assert np.array_equal(val, want) and not np.array_equal(val, np.floor(val))


def test_half_resolution_frames_with_the_source_size_equal_halved_boxes():
    fr = video()
    index, boxes = case_boxes()
    ok = np.isfinite(boxes).all(1) & (np.abs(boxes) < 1e29).all(1)
    boxes = boxes[ok] * np.float32(2)                                                    # exact
    val, valid = crop_values(fr, index[ok], boxes, (7, 5), source_size=(2 * H, 2 * W), samples=2)
    want, want_valid = crop_values(fr, index[ok], boxes * np.float32(0.5), (7, 5), samples=2)
    assert np.array_equal(val, want) and np.array_equal(valid, want_valid)


# ------------------------------------------------------------------------------------------------------------------------------
# against grid_sample
# ------------------------------------------------------------------------------------------------------------------------------
def grid_sample_reference(fr, index, boxes, size, source_size, scale, s):
    """the mean of the s x s sub-grid samples taken by fp64 ``grid_sample(bilinear, border, align_corners=False)``"""
    (h, w), (H_, W_) = size, fr.shape[1:3]
    H0, W0 = source_size
    out = []
    for n, b in zip(index, boxes.astype(np.float64)):
        cx, cy, bw, bh = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, (b[2] - b[0]) * scale, (b[3] - b[1]) * scale
        u = ((cx - bw / 2) + (np.arange(w * s) + 0.5) * bw / (w * s)) * W_ / W0              # continuous frame coordinates
        v = ((cy - bh / 2) + (np.arange(h * s) + 0.5) * bh / (h * s)) * H_ / H0
        grid = torch.from_numpy(np.stack(np.meshgrid(u / W_ * 2 - 1, v / H_ * 2 - 1), -1)[None])
        img = torch.from_numpy(fr[n]).permute(2, 0, 1)[None].double()
        got = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0).numpy()
        out.append(got.reshape(h, s, w, s, 3).mean((1, 3)))
    return np.stack(out)


@pytest.mark.parametrize("samples", (1, 3))
@pytest.mark.parametrize("source_size,scale", (((H, W), 1.0), ((100, 141), 1.5)))
def test_crop_values_against_fp64_grid_sample(samples, source_size, scale):
    fr = video()
    index, boxes = case_boxes()
    ok = (index >= 0) & (index < N) & np.isfinite(boxes).all(1) & (np.abs(boxes) < 1e29).all(1)
    index, boxes = index[ok], boxes[ok]
    assert len(boxes) >= 14 and (boxes[:, 0] < 0).any() and (boxes[:, 2] > W).any() and (boxes[:, 1] < 0).any() and (boxes[:, 3] > H).any()
    val, valid = crop_values(fr, index, boxes, (7, 5), source_size=source_size, scale=scale, samples=samples)
    want = grid_sample_reference(fr, index, boxes, (7, 5), source_size, scale, samples)
    err = float(np.abs(val - want).max())
    print("max |crop_values - grid_sample| = %.3g" % err)
    assert valid.all() and err <= 1e-9


# ------------------------------------------------------------------------------------------------------------------------------
# invalid rows, crop_table, the host path
# ------------------------------------------------------------------------------------------------------------------------------
def test_invalid_rows_are_zero_and_leave_their_neighbours_alone():
    fr = video()
    nan, inf = float("nan"), float("inf")
    good = (5.3, 4.1, 30.7, 33.2)
    index = [0, -1, 1, N, 2, 0, 1, 2, 0]
    boxes = f32([good, good, good, good, good, (nan, 1, 5, 9), good, (1, 2, inf, 9), (1, -inf, 4, 9)])
    pix, valid = crop_rows(fr, index, boxes, (7, 5), samples=2)
    val, valid_v = crop_values(fr, index, boxes, (7, 5), samples=2)
    assert valid.tolist() == valid_v.tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 0] and valid.dtype == np.uint8
    for r in np.nonzero(valid == 0)[0]:
        assert not pix[r].any() and not val[r].any()
    for r in np.nonzero(valid)[0]:
        alone, _ = crop_rows(fr, [index[r]], boxes[r:r + 1], (7, 5), samples=2)
        assert pix[r].any() and np.array_equal(pix[r], alone[0])
    for bad in (dict(samples=0), dict(samples=5), dict(samples=1.5), dict(scale=0.0), dict(scale=-1.0), dict(scale=inf), dict(scale=nan)):
        with pytest.raises(ValueError):
            crop_rows(fr, [0], f32([good]), (7, 5), **bad)
    with pytest.raises(ValueError):
        crop_rows(fr, [0], f32([good]), (0, 5))
    empty, valid = crop_rows(fr, [], np.zeros((0, 4), np.float32), (7, 5))
    assert empty.shape == (0, 7, 5, 3) and valid.shape == (0,)


def test_crop_table_of_tubes_and_tracks_dense_or_not(capsys):
    vd, va = padded_detections(), padded_actors()
    for tubes in (vd.tubes(), vd.tubes(dense=True), va.tracks(), va.tracks(dense=True)):
        index, boxes, offsets = crop_table(tubes)
        assert index.dtype == np.int32 and boxes.dtype == np.float32 and offsets.dtype == np.int64 and boxes.shape == (len(index), 4)
        assert offsets[0] == 0 and offsets[-1] == len(index) and len(offsets) == len(tubes) + 1 and len(tubes) >= 2
        for i, t in enumerate(tubes):
            a, b = offsets[i], offsets[i + 1]
            assert index[a:b].tolist() == list(t["frames"]) and boxes[a:b].tobytes() == np.asarray(t["boxes"], np.float32).tobytes()
    assert len(crop_table(vd.tubes(dense=True))[0]) > len(crop_table(vd.tubes())[0])
    index, boxes, offsets = crop_table([])
    assert index.shape == (0,) and boxes.shape == (0, 4) and offsets.tolist() == [0]
    with pytest.raises(ValueError, match="tube 0"):
        crop_table([dict(frames=[1, 2], boxes=np.zeros((3, 4), np.float32))])
    capsys.readouterr()


def test_tube_crops_on_a_cpu_tensor_is_the_definition_and_says_so(capsys):
    fr = video(1, (60, H, W))
    tubes = padded_detections().tubes(dense=True)
    capsys.readouterr()
    index, boxes, offsets = crop_table(tubes)
    for frames in (torch.from_numpy(fr), fr):
        got = tube_crops(frames, tubes, (7, 5), source_size=(80, 120), scale=1.25, samples=2)
        err = capsys.readouterr().err
        assert err.count("\n") == 1 and "tube_crops" in err and "on the host" in err and "CPU" in err
        want, valid = crop_rows(fr, index, boxes, (7, 5), source_size=(80, 120), scale=1.25, samples=2)
        assert isinstance(got, TubeCrops) and got.path == "host" and len(got) == len(tubes) and np.array_equal(got.offsets, offsets)
        assert got.pixels.dtype == torch.uint8 and np.array_equal(got.pixels.numpy(), want) and np.array_equal(got.valid.numpy(), valid) and want.any()
        for i in range(len(tubes)):
            assert np.array_equal(got[i].numpy(), want[offsets[i]:offsets[i + 1]]) and got[i].shape[0] == len(tubes[i]["frames"])
        assert np.array_equal(got[-1].numpy(), got[len(tubes) - 1].numpy())
        with pytest.raises(IndexError):
            got[len(tubes)]
        pixels, host_valid = got.to_host()
        assert np.array_equal(pixels, want) and np.array_equal(host_valid, valid)
    table = tube_crops(fr, tubes, (7, 5), normalize=True)
    capsys.readouterr()
    want, _ = crop_rows(fr, index, boxes, (7, 5))
    assert table.pixels.dtype == torch.float32 and tuple(table.pixels.shape) == (len(index), 3, 7, 5)
    assert table.pixels.numpy().tobytes() == normalized(want, ip.normalize_lut()).tobytes()
    assert np.array_equal(table.pixels.numpy()[:, 1], ip.normalize_lut()[1][want[..., 1]])
    none = tube_crops(fr, [], (7, 5))
    assert len(none) == 0 and tuple(none.pixels.shape) == (0, 7, 5, 3)
    with pytest.raises(ValueError):
        tube_crops(fr.astype(np.float32), tubes, (7, 5))
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------------
# settings, the C ABI, signatures
# ------------------------------------------------------------------------------------------------------------------------------
def test_crop_settings():
    cfg = get_cfg_defaults()
    assert crop_settings(cfg) == dict(size=(112, 112), scale=1.0, samples=1)
    cfg.CONFIG.VAL.CROPS.SIZE, cfg.CONFIG.VAL.CROPS.SCALE, cfg.CONFIG.VAL.CROPS.SAMPLES = [64, 32], 2, 4
    assert crop_settings(cfg) == dict(size=(64, 32), scale=2.0, samples=4)
    bad = dict(SIZE=(112, [112], [112, 0], [112, 112, 3], [112.0, 112], [True, 2], "112", None), SCALE=(0, -1.0, float("nan"), float("inf"), "1", None, True),
               SAMPLES=(0, 5, 1.0, True, None, "2", -1))
    for key, values in bad.items():
        for v in values:
            cfg = get_cfg_defaults()
            cfg.CONFIG.VAL.CROPS[key] = v
            with pytest.raises(ValueError, match=r"CONFIG\.VAL\.CROPS\.%s " % key):
                crop_settings(cfg)
    paths = sorted(glob.glob(os.path.join(ROOT, "configuration", "*.yaml")))
    assert len(paths) == 4
    for p in paths:
        assert crop_settings(load_cfg(p)) == dict(size=(112, 112), scale=1.0, samples=1)


def test_tuber_tube_crops_is_declared_and_exported():
    declared = {name: (ret, args) for ret, name, args in lib.header_prototypes()}
    for name in ("tuber_tube_crops", "tuber_tube_crops_limits"):
        assert name in declared and hasattr(lib.load(), name)
    ret, args = declared["tuber_tube_crops"]
    assert ret == "int" and [a[1] for a in args] == ["frames", "N", "H", "W", "frame_index", "boxes", "R", "h", "w", "fx", "fy", "scale", "samples", "lut", "out",
                                                     "valid", "stream"]
    assert [a[0] for a in args[9:12]] == ["double"] * 3 and args[0][0] == "const unsigned char*" and args[14][0] == "void*" and args[-1][0] == "hipStream_t"
    assert lib.query("tuber_tube_crops_limits", 2) == 4
    assert lib.query("tuber_tube_crops_limits", 0) > 0 and lib.query("tuber_tube_crops_limits", 1) > 0 and lib.query("tuber_tube_crops_limits", 3) == -1


def test_keep_video_is_off_by_default_and_crops_needs_it(capsys):
    assert inspect.signature(VideoDetector.__init__).parameters["keep_video"].default is False
    assert "keep_video" not in inspect.signature(VideoStream.__init__).parameters
    assert [p.default for p in list(inspect.signature(VideoDetections.crops).parameters.values())[2:]] == [None, None, None, False]
    assert "keep_video" in VideoStream.__doc__ and "stays allocated" in VideoDetector.__doc__
    vd = padded_detections()
    assert vd.video is None and vd.source_size is None
    with pytest.raises(RuntimeError, match="keep_video=True"):
        vd.crops(vd.tubes())
    vd.video, vd.source_size = torch.from_numpy(video(1, (60, H, W))), (80, 120)        # what VideoDetector(..., keep_video=True) sets
    capsys.readouterr()
    got = vd.crops(vd.tubes(dense=True), size=(7, 5))
    want, _ = crop_rows(vd.video.numpy(), *crop_table(vd.tubes(dense=True))[:2], (7, 5), source_size=(80, 120))
    assert got.path == "host" and np.array_equal(got.pixels.numpy(), want)
    assert tuple(vd.crops(vd.tubes()).pixels.shape[1:]) == (112, 112, 3)                # CONFIG.VAL.CROPS' defaults
    capsys.readouterr()
