"""Deterministic synthetic weights, clips and targets.

There are no checkpoints or datasets in this image, so parity and throughput
runs use:

* **name-hashed weights** -- every tensor of a ``state_dict`` is filled from a CPU
  generator seeded with ``crc32(name)``, so the reference model (imported only when
  generating golden vectors), the CPU oracle and the HIP model get bit-identical
  weights without sharing construction order;
* **synthetic clips** -- ``randn`` (ImageNet-normalised frames are ~N(0,1));
* **synthetic targets** following the target-dict contract of
  ``datasets/ava_frame.py:112-128`` / ``datasets/jhmdb_frame.py:170-189``.
"""
import zlib

import torch


def _gen(name, salt=0):
    g = torch.Generator(device="cpu")
    g.manual_seed((zlib.crc32(name.encode()) + 7919 * salt) & 0x7FFFFFFF)
    return g


# "spread" fixture (round 5): at plain name-hashed weights the DETR decoder's queries are near-copies of each other -- the random
# encoder averages its tokens into one common vector (memory diversity over tokens 0.08), every query attends almost uniformly, and
# the 15 tubelet queries' boxes differ by <= 1.7e-3, their actor probabilities by 0.06: below bf16 noise, so no bf16 execution can
# reproduce the reference's Hungarian assignment or move a post-processing gate.  These gains (found by measurement on the fp32
# oracle, oracle/gen_golden.py) keep the tokens and the queries apart: identity-dominated encoder layers, sharper attention, larger
# query embeddings, wider actor / box heads.  With them the queries' decoder states differ by ~30 % of their norm (was 0.3 %).
SPREAD_GAINS = {"encoder_residual": 0.1,      # transformer.encoder.layers.*.{self_attn.out_proj, linear2}.{weight, bias}
                "attention_qk": 2.0,          # q / k rows of every transformer.* in_proj_{weight, bias}: scores x 4
                "query_embed": 3.0,
                "class_embed_b": 3.0,         # actor logits: p_b spreads over ~[0.05, 0.95]
                "bbox_last": 2.0}             # bbox_embed.layers.2.weight: boxes spread over >= 0.05 without saturating the sigmoid


def _spread_gain(key, v):
    g = SPREAD_GAINS
    if key.startswith("transformer.encoder.") and key.rsplit(".", 1)[0].endswith(("self_attn.out_proj", "linear2")):
        return v * g["encoder_residual"]
    if key.startswith("transformer.") and key.endswith(("in_proj_weight", "in_proj_bias")):
        v = v.clone()
        v[: 2 * v.shape[0] // 3] *= g["attention_qk"]
        return v
    if key == "query_embed.weight":
        return v * g["query_embed"]
    if key == "class_embed_b.weight":
        return v * g["class_embed_b"]
    if key == "bbox_embed.layers.2.weight":
        return v * g["bbox_last"]
    return v


@torch.no_grad()
def name_hashed_state(state_dict, salt=0, residual_gain=None, spread=False):
    """Return ``{name: tensor}`` with deterministic values for every entry of ``state_dict``.

    Rules (by leaf name): BN/LN ``weight`` ~ 1 + 0.1 N, ``bias`` ~ 0.1 N (0.02 N for
    conv/linear biases), ``running_mean`` ~ 0.1 N, ``running_var`` ~ 1 + 0.2 U,
    ``num_batches_tracked`` = 0, embeddings ~ N, every >=2-D weight ~ N(0, 1/fan_in).
    A leading ``module.`` (DDP prefix) is ignored so wrapped and bare models agree.

    ``residual_gain``: scale every ``bn4.weight`` -- the last BatchNorm of each residual branch (ir_CSN_152.py:64,82-84) -- by this
    factor.  At random weights a 50-bottleneck training-mode-BatchNorm body amplifies bf16 rounding through ReLU-mask flips until even
    an ideally-accumulated bf16 execution decorrelates from fp32; with identity-dominated blocks (gain ~0.05-0.1) the deep gradient
    stays well-conditioned, which is what a parity test at real depth needs (tests/test_fullsize_gpu.py).

    ``spread``: apply ``SPREAD_GAINS`` (non-degenerate tubelet queries; see there).
    """
    out = {}
    for name, t in state_dict.items():
        key = name[7:] if name.startswith("module.") else name
        g = _gen(key, salt)
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            v = torch.zeros_like(t)
        elif leaf == "running_mean":
            v = 0.1 * torch.randn(t.shape, generator=g)
        elif leaf == "running_var":
            v = 1.0 + 0.2 * torch.rand(t.shape, generator=g)
        elif leaf == "empty_weight":
            v = t.clone()
        elif t.dim() >= 2:
            if "query_embed" in key or "query_pool" in key:
                v = torch.randn(t.shape, generator=g)
            else:
                fan_in = t[0].numel()
                v = torch.randn(t.shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif leaf == "weight":            # 1-D weight: BatchNorm / LayerNorm gamma
            v = 1.0 + 0.1 * torch.randn(t.shape, generator=g)
            if residual_gain is not None and key.endswith(".bn4.weight"):
                v = v * float(residual_gain)
        elif leaf in ("bias", "in_proj_bias"):
            is_norm = any(s in key for s in (".bn", "norm", "down_sample.1"))
            v = (0.1 if is_norm else 0.02) * torch.randn(t.shape, generator=g)
        else:
            v = 0.02 * torch.randn(t.shape, generator=g)
        if spread:
            v = _spread_gain(key, v)
        out[name] = v.to(t.dtype)
    return out


@torch.no_grad()
def load_name_hashed(module, salt=0, residual_gain=None, spread=False):
    """Fill ``module``'s parameters and buffers in place with name-hashed values."""
    sd = module.state_dict()
    vals = name_hashed_state(sd, salt, residual_gain, spread)
    for k, t in sd.items():
        t.copy_(vals[k].to(t.device))
    return module


def synthetic_clips(batch, t, h, w, seed=1234, device="cpu", sizes=None):
    """``batch`` clips (3,t,h,w) ~ N(0,1).  ``sizes`` = per-clip (h,w) for ragged batches."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    if sizes is None:
        return torch.randn(batch, 3, t, h, w, generator=g).to(device)
    return [torch.randn(3, t, hh, ww, generator=g).to(device) for hh, ww in sizes]


def structured_clips(batch, t, h, w, seed=1234, amp=2.0, device="cpu"):
    """Clips with spatial / temporal structure: 0.5 N(0,1) pixel noise + ``amp`` x a trilinearly upsampled coarse random field (one
    value per 16 x 16 pixel cell and 8 frames).  i.i.d. noise gives every backbone position statistically the same content, so
    the feature map (and with it what the queries can attend to) barely varies over positions; this does."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    base = torch.randn(batch, 3, t, h, w, generator=g)
    coarse = torch.randn(batch, 3, 4, max(2, h // 16), max(2, w // 16), generator=g)
    low = torch.nn.functional.interpolate(coarse, size=(t, h, w), mode="trilinear", align_corners=False)
    return (0.5 * base + amp * low).to(device)


def synthetic_targets(batch, dataset="ava", num_classes=80, seed=4321, device="cpu", hw=(256, 340),
                      boxes_per_clip=None):
    """Target dicts with the keys the criterion reads.

    AVA: ``boxes`` float32 [N,5] = (key_t=16, cx, cy, w, h) in [0,1]; ``labels`` float32 [N,80]
    multi-hot.  JHMDB: ``labels`` int64 [N], ``vis`` int64 [1], ``key_pos`` int64 scalar (=16).
    """
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    out = []
    for b in range(batch):
        if dataset == "ava":
            n = int(torch.randint(1, 4, (1,), generator=g)) if boxes_per_clip is None else boxes_per_clip[b]
        else:
            n = 1
        cxcy = 0.3 + 0.4 * torch.rand(n, 2, generator=g)
        wh = 0.1 + 0.2 * torch.rand(n, 2, generator=g)
        boxes = torch.cat([torch.full((n, 1), 16.0), cxcy, wh], dim=1)
        t = {"boxes": boxes.to(device),
             "size": torch.tensor(list(hw), dtype=torch.int64, device=device),
             "orig_size": torch.tensor(list(hw), dtype=torch.int64, device=device),
             "area": (wh[:, 0] * wh[:, 1] * hw[0] * hw[1]).to(device)}
        if dataset == "ava":
            lab = (torch.rand(n, num_classes, generator=g) < 0.05).float()
            lab[:, 11] = 1.0
            t["labels"] = lab.to(device)
        else:
            t["labels"] = torch.randint(0, num_classes, (n,), generator=g).to(device)
            t["vis"] = torch.ones(1, dtype=torch.int64, device=device)
            t["key_pos"] = torch.tensor(16, dtype=torch.int64, device=device)
        out.append(t)
    return out


def zero_dropout(model):
    """Deterministic train mode for parity runs: nn.Dropout.p and nn.MultiheadAttention.dropout -> 0."""
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(getattr(m, "dropout", None), float):
            m.dropout = 0.0
    return model


def synthetic_frame_map_case(frames, dets=15, classes=80, seed=7, max_gt=5, gated=0.0, hw=(64, 96)):
    """A synthetic validation result for the frame-mAP evaluators (evaluation.FrameMAP, device_map.DeviceFrameMAP): ``frames`` frames with
    ``dets`` detection rows each and 0..``max_gt`` ground-truth boxes with 1..3 labels each.  The scores are the distinct values
    ``perm(n * C) / (n * C)`` (n * C < 2^24, so they stay distinct in fp32): no class has two equal scores.  ``gated``: fraction of rows
    whose scores are all 0, like the actor gate of PostProcessAVA -- the only ties then.  About half of the detections sit near a
    ground-truth box (IoU on both sides of 0.5), the rest anywhere.  numpy arrays: ``det_keys`` [n], ``det_boxes`` [n, 4] fp32 xyxy,
    ``det_scores`` [n, C] fp32, ``gt_keys`` [m], ``gt_boxes`` [m, 4] fp64, ``gt_labels`` [m, C] fp64 (0 / 1)."""
    import numpy as np
    n = frames * dets
    assert n * classes < 2 ** 24
    rng = np.random.default_rng(seed)
    H, W = hw
    scores = (rng.permutation(n * classes).astype(np.float64) / (n * classes)).astype(np.float32).reshape(n, classes)
    if gated > 0:
        scores[rng.random(n) < gated] = 0.0
    keys = ["vid%03d_%04d" % (f // 100, 900 + f % 100) for f in range(frames)]
    det_keys, det_boxes, gt_keys, gt_boxes, gt_labels = [], [], [], [], []
    for f in range(frames):
        g = int(rng.integers(0, max_gt + 1))
        xy = rng.uniform(0, 0.6, (g, 2)) * [W, H]
        wh = rng.uniform(0.15, 0.4, (g, 2)) * [W, H]
        gb = np.concatenate([xy, xy + wh], axis=1).astype(np.float32).astype(np.float64)
        for j in range(g):
            lab = np.zeros(classes)
            lab[rng.choice(classes, size=int(rng.integers(1, min(3, classes) + 1)), replace=False)] = 1.0
            gt_keys.append(keys[f]); gt_boxes.append(gb[j]); gt_labels.append(lab)
        for i in range(dets):
            if g and rng.random() < 0.5:
                j = int(rng.integers(0, g))
                box = gb[j] + rng.normal(0, 0.12, 4) * np.tile(gb[j, 2:] - gb[j, :2], 2)
            else:
                p = rng.uniform(0, 0.7, 2) * [W, H]
                box = np.concatenate([p, p + rng.uniform(0.1, 0.3, 2) * [W, H]])
            det_keys.append(keys[f]); det_boxes.append(box)
    return dict(det_keys=det_keys, det_boxes=np.asarray(det_boxes, dtype=np.float32).reshape(n, 4), det_scores=scores, gt_keys=gt_keys,
                gt_boxes=np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), gt_labels=np.asarray(gt_labels, dtype=np.float64).reshape(-1, classes))


def synthetic_frame_map_ucf_case(frames, dets=10, classes=21, seed=7, max_gt=3, tiny=0.05, no_object=0.25, near=0.6, hw=(240, 320)):
    """A synthetic JHMDB / UCF101-24 validation result for evaluation.FrameMAPUCF and device_map.DeviceFrameMAPUCF: ``frames`` frames with
    ``dets`` rows of ``classes + 1`` probabilities (the classes, then no-object) that sum to 1 and 0..``max_gt`` ground-truth boxes of one
    class each.  The top value of row r is the fp32 number ``0.5 + 0.45 * (perm(n)[r] + 1) / (n + 1)``: distinct (their spacing is far above
    an fp32 ulp), above 0.5 and therefore above every other entry of the row, so the arg-max is unambiguous, survives fp32 rounding, and no
    class has two equal scores.  About ``no_object`` of the rows have no-object on top, about ``tiny`` of the ground-truth boxes measure
    3 x 3 = 9 px^2 (their frame goes on the exclude list), about ``near`` of the detections sit near a ground-truth box of their frame (IoU
    on both sides of 0.5) and mostly carry its class.  numpy arrays: ``det_keys`` [n], ``det_boxes`` [n, 4] fp32 xyxy, ``det_probs``
    [n, C + 1] fp32, ``gt_keys`` [m], ``gt_boxes`` [m, 4] fp64, ``gt_labels`` [m, max(21, C)] fp64 one-hot."""
    import numpy as np
    n, C = frames * dets, classes
    rng = np.random.default_rng(seed)
    H, W = hw
    width = max(21, C)
    top = (0.5 + 0.45 * (rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    keys = ["clip%03d_%05d" % (f // 40, 1 + f % 40) for f in range(frames)]
    det_keys, det_boxes, det_top, gt_keys, gt_boxes, gt_labels = [], [], [], [], [], []
    for f in range(frames):
        g = int(rng.integers(0, max_gt + 1))
        xy = rng.uniform(0, 0.6, (g, 2)) * [W, H]
        wh = rng.uniform(0.15, 0.4, (g, 2)) * [W, H]
        gb = np.concatenate([xy, xy + wh], axis=1).astype(np.float32).astype(np.float64)
        gc = rng.integers(0, C, g)
        for j in range(g):
            if rng.random() < tiny:
                gb[j, 2:] = gb[j, :2] + 3.0
            lab = np.zeros(width)
            lab[gc[j]] = 1.0
            gt_keys.append(keys[f]); gt_boxes.append(gb[j].copy()); gt_labels.append(lab)
        for i in range(dets):
            a = int(rng.integers(0, C))
            if g and rng.random() < near:
                j = int(rng.integers(0, g))
                box = gb[j] + rng.normal(0, 0.1, 4) * np.tile(gb[j, 2:] - gb[j, :2], 2)
                if rng.random() < 0.8:
                    a = int(gc[j])
            else:
                p = rng.uniform(0, 0.7, 2) * [W, H]
                box = np.concatenate([p, p + rng.uniform(0.1, 0.3, 2) * [W, H]])
            if rng.random() < no_object:
                a = C
            det_keys.append(keys[f]); det_boxes.append(box); det_top.append(a)
    rest = rng.uniform(0.05, 1.0, (n, C + 1))
    rest[np.arange(n), det_top] = 0.0
    probs = ((1.0 - top.astype(np.float64))[:, None] * rest / rest.sum(axis=1, keepdims=True)).astype(np.float32)
    probs[np.arange(n), det_top] = top
    return dict(det_keys=det_keys, det_boxes=np.asarray(det_boxes, dtype=np.float32).reshape(n, 4), det_probs=probs, gt_keys=gt_keys,
                gt_boxes=np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), gt_labels=np.asarray(gt_labels, dtype=np.float64).reshape(-1, width))


def synthetic_video_map_case(videos, frames, dets=10, classes=24, seed=7, max_tubes=2, drop=0.15, jitter=0.05, echo=0.3, no_object=0.2,
                             hw=(240, 320)):
    """A synthetic JHMDB / UCF101-24 validation result with tubes, for evaluation.VideoMAP and device_map.DeviceVideoMAP: ``videos`` videos of
    ``frames`` frames (keys ``"video%04d-<frame>"``, frames from 1) with exactly ``dets`` rows of ``classes + 1`` probabilities each.  A
    video has 1..``max_tubes`` ground-truth tubes of one class each whose box drifts and breathes smoothly over at least half of the video;
    for every ground-truth box a jittered copy is a detection of (mostly) its class unless it drops out (``drop``: the gaps linking has to
    bridge), about ``echo`` of them come with a second, looser copy (a competing tube), and the remaining rows are spurious boxes that mostly
    score lower.  Top probabilities as ``synthetic_frame_map_ucf_case``: distinct fp32 numbers above 0.5.  numpy arrays: ``det_keys`` [n], ``det_boxes`` [n, 4]
    fp32 xyxy, ``det_probs`` [n, C + 1] fp32, ``gt_keys`` [m], ``gt_boxes`` [m, 4] fp64, ``gt_labels`` [m, max(21, C)] fp64 one-hot,
    ``gt_tubes`` [m] integer tube ids."""
    import numpy as np
    n, C = videos * frames * dets, classes
    rng = np.random.default_rng(seed)
    H, W = hw
    width = max(21, C)
    det_keys, det_boxes, det_top, det_true, gt_keys, gt_boxes, gt_labels, gt_tubes = [], [], [], [], [], [], [], []
    for v in range(videos):
        tubes = []
        for t in range(int(rng.integers(1, max_tubes + 1))):
            span = int(rng.integers((frames + 1) // 2, frames + 1))
            first = int(rng.integers(0, frames - span + 1))
            c0 = rng.uniform(0.25, 0.6, 2) * [W, H]
            tubes.append(dict(id=t, cls=int(rng.integers(0, C)), first=first, last=first + span - 1, c0=c0, vel=rng.uniform(-0.2, 0.2, 2) * [W, H],
                              wh=rng.uniform(0.2, 0.35, 2) * [W, H], phase=rng.uniform(0, 6.28)))
        for f in range(frames):
            key = "video%04d-%d" % (v, f + 1)
            rows = []
            for t in tubes:
                if not t["first"] <= f <= t["last"]:
                    continue
                u = f / max(frames - 1, 1)
                ctr = t["c0"] + t["vel"] * u
                wh = t["wh"] * (1.0 + 0.15 * np.sin(t["phase"] + 6.28 * u))
                gb = np.concatenate([ctr - wh / 2, ctr + wh / 2]).astype(np.float32).astype(np.float64)
                lab = np.zeros(width)
                lab[t["cls"]] = 1.0
                gt_keys.append(key); gt_boxes.append(gb); gt_labels.append(lab); gt_tubes.append(t["id"])
                if rng.random() >= drop:
                    rows.append((gb + rng.normal(0, jitter, 4) * np.tile(wh, 2), t["cls"] if rng.random() < 0.9 else int(rng.integers(0, C)), 1))
                    if rng.random() < echo:
                        rows.append((gb + rng.normal(0, 3 * jitter, 4) * np.tile(wh, 2), t["cls"], 0))
            rows = rows[:dets]
            while len(rows) < dets:
                p = rng.uniform(0, 0.7, 2) * [W, H]
                rows.append((np.concatenate([p, p + rng.uniform(0.1, 0.3, 2) * [W, H]]), C if rng.random() < no_object else int(rng.integers(0, C)), 0))
            for i in rng.permutation(dets):
                det_keys.append(key); det_boxes.append(rows[i][0]); det_top.append(rows[i][1]); det_true.append(rows[i][2])
    # the copies of the ground truth mostly outrank the rest: a noisy rank, then distinct values as synthetic_frame_map_ucf_case has them
    rank = np.argsort(np.argsort(np.asarray(det_true) * 0.5 + rng.uniform(0, 1, n), kind="stable"), kind="stable")
    top = (0.5 + 0.45 * (rank + 1.0) / (n + 1.0)).astype(np.float32)
    rest = rng.uniform(0.05, 1.0, (n, C + 1))
    rest[np.arange(n), det_top] = 0.0
    probs = ((1.0 - top.astype(np.float64))[:, None] * rest / rest.sum(axis=1, keepdims=True)).astype(np.float32)
    probs[np.arange(n), det_top] = top
    return dict(det_keys=det_keys, det_boxes=np.asarray(det_boxes, dtype=np.float32).reshape(n, 4), det_probs=probs, gt_keys=gt_keys,
                gt_boxes=np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), gt_labels=np.asarray(gt_labels, dtype=np.float64).reshape(-1, width),
                gt_tubes=np.asarray(gt_tubes, dtype=np.int64))
