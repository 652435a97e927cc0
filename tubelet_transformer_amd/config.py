"""Minimal yacs-compatible config node for the TubeR hot path.

The reference drives everything from a yacs ``CfgNode`` built by
``pipelines/video_action_recognition_config.py:5-222`` (``get_cfg_defaults``)
and ``cfg.merge_from_file(yaml)`` (``train_tuber_ava.py:100-101``).  yacs is not
installed in this image, so this module provides the subset of its behaviour the
hot path relies on: attribute access, ``merge_from_file``, ``merge_from_other``,
``clone``, ``dump``, ``freeze``/``defrost``, ``new_allowed`` sub-trees, and
yacs' habit of ``literal_eval``-ing YAML strings (so ``LR: 1e-4`` becomes a float).
"""
import ast
import copy

import yaml


class CfgNode(dict):
    _FROZEN = "__frozen__"
    _NEW_ALLOWED = "__new_allowed__"

    def __init__(self, init=None, new_allowed=False):
        super().__init__()
        self.__dict__[CfgNode._FROZEN] = False
        self.__dict__[CfgNode._NEW_ALLOWED] = new_allowed
        for k, v in (init or {}).items():
            self[k] = CfgNode(v, new_allowed=new_allowed) if isinstance(v, dict) and not isinstance(v, CfgNode) else v

    # attribute access -------------------------------------------------
    def __getattr__(self, name):
        if name in self:
            return self[name]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if self.__dict__[CfgNode._FROZEN]:
            raise AttributeError("Attempted to set {} to {}, but CfgNode is immutable".format(name, value))
        self[name] = value

    # yacs API -----------------------------------------------------------
    def is_frozen(self):
        return self.__dict__[CfgNode._FROZEN]

    def is_new_allowed(self):
        return self.__dict__[CfgNode._NEW_ALLOWED]

    def _set_frozen(self, flag):
        self.__dict__[CfgNode._FROZEN] = flag
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_frozen(flag)

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def clone(self):
        return copy.deepcopy(self)

    def __deepcopy__(self, memo):
        out = CfgNode(new_allowed=self.is_new_allowed())
        for k, v in self.items():
            out[k] = copy.deepcopy(v, memo)
        return out

    def to_dict(self):
        return {k: (v.to_dict() if isinstance(v, CfgNode) else (list(v) if isinstance(v, tuple) else v))
                for k, v in self.items()}

    def dump(self, **kwargs):
        return yaml.safe_dump(self.to_dict(), **kwargs)

    def merge_from_file(self, cfg_filename):
        with open(cfg_filename, "r") as f:
            loaded = yaml.safe_load(f)
        self.merge_from_other_cfg(loaded)

    def merge_from_other_cfg(self, other):
        _merge(other, self, [])

    def merge_from_list(self, cfg_list):
        assert len(cfg_list) % 2 == 0, "Override list has odd length: {}".format(cfg_list)
        for full_key, v in zip(cfg_list[0::2], cfg_list[1::2]):
            node = self
            parts = full_key.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = _decode(v)


def _decode(v):
    """yacs ``_decode_cfg_value``: dict -> node, str -> literal_eval if it parses."""
    if isinstance(v, dict):
        return CfgNode(v, new_allowed=True)
    if not isinstance(v, str):
        return v
    try:
        return ast.literal_eval(v)
    except (ValueError, SyntaxError):
        return v


def _merge(src, dst, path):
    for k, v in src.items():
        full = ".".join(path + [k])
        v = _decode(v) if not isinstance(v, dict) else v
        if k in dst:
            if isinstance(dst[k], CfgNode) and isinstance(v, dict):
                _merge(v, dst[k], path + [k])
            else:
                if isinstance(dst[k], tuple) and isinstance(v, list):
                    v = tuple(v)
                if isinstance(dst[k], float) and isinstance(v, int):
                    v = float(v)
                dst[k] = CfgNode(v, new_allowed=True) if isinstance(v, dict) else v
        elif dst.is_new_allowed():
            dst[k] = CfgNode(v, new_allowed=True) if isinstance(v, dict) else v
        else:
            raise KeyError("Non-existent config key: {}".format(full))


def get_cfg_defaults():
    """Defaults for the keys the TubeR hot path reads.

    Mirrors the relevant subset of ``pipelines/video_action_recognition_config.py``
    (DDP_CONFIG ``:11-31``, CONFIG.* nodes with ``new_allowed=True`` ``:37-39,105,178,202``)
    plus the hot-path keys every published YAML supplies, with the values of
    ``configuration/TubeR_CSN152_AVA21.yaml`` as defaults so a partial YAML still builds.
    """
    C = CfgNode()
    C.DDP_CONFIG = CfgNode(dict(
        WORLD_SIZE=1, WORLD_RANK=0, GPU_WORLD_SIZE=8, GPU_WORLD_RANK=0,
        DIST_URL="tcp://127.0.0.1:10001", WOLRD_URLS=["127.0.0.1"], AUTO_RANK_MATCH=True,
        DIST_BACKEND="nccl", GPU=0, DISTRIBUTED=True))
    cfg = CfgNode(new_allowed=True)
    cfg.EVAL_ONLY = False
    cfg.TWO_STREAM = False
    cfg.USE_LFB = False
    cfg.USE_LOCATION = False
    cfg.TRAIN = CfgNode(dict(
        START_EPOCH=0, EPOCH_NUM=20, BATCH_SIZE=2, LR=1e-4, MIN_LR=1e-5, LR_BACKBONE=1e-5,
        W_DECAY=1e-4, LR_POLICY="step", AUX_LOSS=True,
        ACCUM_STEPS=1,                         # micro-batches per optimizer step (accum.py; not a reference key)
        # weight averaging inside the training step (weight_avg.py; not reference keys): MODE ema | swa, updates at the optimizer steps
        # t >= START with (t - START) % PERIOD == 0, EVAL: validate with the averaged weights
        EMA=dict(ENABLE=False, MODE="ema", DECAY=0.9999, WARMUP=False, START=0, PERIOD=1, EVAL=True),
        # per-tensor gradient / parameter / update statistics inside the training step (monitor.py; not reference keys): a row every EVERY
        # optimizer steps, the last HISTORY rows kept on the device
        MONITOR=dict(ENABLE=False, EVERY=50, HISTORY=8)), new_allowed=True)
    cfg.VAL = CfgNode(dict(
        FREQ=2, BATCH_SIZE=1,
        # frame-mAP of validate_tuber_detection (AVA) and validate_tuber_ucf_detection (JHMDB / UCF101-24) computed on the device
        # (device_map.py; not reference keys): ENABLE keeps detections and ground truth in device buffers and runs the frame_map.hip
        # kernels instead of the host FrameMAP / FrameMAPUCF over the result files; FILES: the per-rank result files are written as
        # well (reference format), False: no file, no host copy of the detections
        DEVICE_MAP=dict(ENABLE=False, FILES=True),
        # video-mAP of validate_tuber_ucf_detection over linked action tubes (evaluation.VideoMAP / device_map.DeviceVideoMAP; not reference
        # keys): consecutive detections of a class link when their IoU is at least LINK_IOU, over at most MAX_GAP empty frames; tubes shorter
        # than MIN_LEN are not counted; THRESHOLDS: spatio-temporal IoU thresholds, "0.5:0.95" the mean over 0.50, 0.55, ..., 0.95; DENSE: the
        # default of tubes(dense=) / tracks(dense=) of video.py -- a box on every frame of a tube's extent, interpolated between the linked key
        # detections (evaluation.dense_rows / tuber_tube_dense); no part of video-mAP
        VIDEO_MAP=dict(ENABLE=False, LINK_IOU=0.2, MAX_GAP=2, MIN_LEN=1, THRESHOLDS=[0.2, 0.5, 0.75, "0.5:0.95"], DENSE=False),
        # ranked detections decoded on the device (detect.Detector; not reference keys): a candidate scores at least SCORE_THR, the best TOPK
        # per clip are kept; ACTOR_THR: the actor-probability gate of the AVA rule (the reference's 0.8)
        DETECT=dict(SCORE_THR=0.05, TOPK=100, ACTOR_THR=0.8),
        # actor tracks of an AVA video (detect.Detector(actors=...), video.VideoActors.tracks; not reference keys): the best TOPK actors of a key
        # frame are kept, linked class-agnostically (LINK_IOU, MAX_GAP, MIN_LEN as in VIDEO_MAP), a row's action scores smoothed over the rows of
        # its track at most WINDOW key frames away, a track labelled with the classes whose mean score is at least LABEL_THR.  None: TOPK =
        # min(MODEL.QUERY_NUM, 64 active tubes // (MAX_GAP + 1)), LINK_IOU / MAX_GAP / MIN_LEN = VIDEO_MAP's, LABEL_THR = DETECT.SCORE_THR
        ACTORS=dict(TOPK=None, LINK_IOU=None, MAX_GAP=None, MIN_LEN=None, WINDOW=1, LABEL_THR=None),
        # spatio-temporal NMS over linked tubes (evaluation.tube_nms / tuber_tube_nms; not reference keys): per (video, class) a tube whose
        # spatio-temporal IoU with a higher-scored kept tube exceeds IOU is dropped -- before video-mAP in validate_tuber_ucf_detection and in
        # video.VideoDetections.tubes(); ACTORS_IOU: the same, class-agnostic, for video.VideoActors.tracks().  None: off.  0.3 is customary
        TUBE_NMS=dict(IOU=None, ACTORS_IOU=None),
        # crops of tubes and actor tracks out of the resident video (crops.py / tuber_tube_crops; not reference keys): the defaults of
        # video.VideoDetections.crops() -- SIZE (h, w) of a crop, SCALE enlarges a box about its centre, SAMPLES: every output pixel is the mean
        # of SAMPLES x SAMPLES bilinear samples (RoIAlign's sampling_ratio)
        CROPS=dict(SIZE=[112, 112], SCALE=1.0, SAMPLES=1),
        # both validation loops run the eval forward as a captured hipGraph per input shape (detect.GraphedEval; not a reference key)
        GRAPHED=False), new_allowed=True)
    cfg.DATA = CfgNode(dict(
        DATASET_NAME="ava", NUM_CLASSES=80, IMG_SIZE=256, TEMP_LEN=32, FRAME_RATE=2), new_allowed=True)
    cfg.MODEL = CfgNode(dict(
        NAME="", SINGLE_FRAME=True, BACKBONE_NAME="CSN-152", TEMPORAL_DS_STRATEGY="avg", LAST_STRIDE=False,
        GENERATE_LFB=False, ENC_LAYERS=6, DEC_LAYERS=6, D_MODEL=256, NHEAD=8, DIM_FEEDFORWARD=2048,
        QUERY_NUM=15, NORMALIZE_BEFORE=False, DROPOUT=0.1, DS_RATE=8, TEMP_LEN=32, PRETRAINED=False,
        PRETRAIN_BACKBONE_DIR="", PRETRAIN_TRANSFORMER_DIR="", PRETRAINED_PATH="", LOAD=False, LOAD_FC=True,
        FREEZE_BN="none"),      # backbone BatchNorm layers kept in eval mode while training: none | frozen | all (bn_stats.py; not a reference key)
        new_allowed=True)
    cfg.MATCHER = CfgNode(dict(COST_CLASS=12, COST_BBOX=5, COST_GIOU=2, BNY_LOSS=True, BEFORE=False),
                          new_allowed=True)
    cfg.LOSS_COFS = CfgNode(dict(
        MASK_COF=1, DICE_COF=12, BBOX_COF=5, GIOU_COF=2, EOS_COF=0.1, WEIGHT=10, WEIGHT_CHANGE=1000,
        LOSS_CHANGE_COF=2, CLIPS_MAX_NORM=0.1), new_allowed=True)
    cfg.LOG = CfgNode(dict(BASE_PATH="", EXP_NAME="use_time", LOG_DIR="tb_log", SAVE_DIR="checkpoints",
                           EVAL_DIR="", SAVE_FREQ=1, RES_DIR="tmp"), new_allowed=True)
    C.CONFIG = cfg
    return C


def video_map_settings(cfg):
    """CONFIG.VAL.VIDEO_MAP validated -> the keyword arguments of ``VideoMAP`` / ``DeviceVideoMAP``; a bad value raises ValueError naming its key"""
    vm = cfg.CONFIG.VAL.VIDEO_MAP

    def bad(key, why):
        raise ValueError("CONFIG.VAL.VIDEO_MAP.%s = %r: %s" % (key, vm[key], why))
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    if not isinstance(vm.ENABLE, bool):
        bad("ENABLE", "must be True or False")
    if not isinstance(vm.DENSE, bool):
        bad("DENSE", "must be True or False")
    if not number(vm.LINK_IOU) or not 0.0 <= vm.LINK_IOU <= 1.0:
        bad("LINK_IOU", "must be a number in [0, 1]")
    if not isinstance(vm.MAX_GAP, int) or isinstance(vm.MAX_GAP, bool) or vm.MAX_GAP < 0:
        bad("MAX_GAP", "must be an integer >= 0")
    if not isinstance(vm.MIN_LEN, int) or isinstance(vm.MIN_LEN, bool) or vm.MIN_LEN < 1:
        bad("MIN_LEN", "must be an integer >= 1")
    thr = vm.THRESHOLDS
    if not isinstance(thr, (list, tuple)) or len(thr) == 0:
        bad("THRESHOLDS", "must be a non-empty list")
    for t in thr:
        if not (t == "0.5:0.95" or (number(t) and 0.0 < t <= 1.0)):
            bad("THRESHOLDS", 'every entry must be a number in (0, 1] or "0.5:0.95" (got %r)' % (t,))
    if len(set(thr)) != len(thr):
        bad("THRESHOLDS", "entries must be distinct")
    return dict(link_iou=float(vm.LINK_IOU), max_gap=int(vm.MAX_GAP), min_len=int(vm.MIN_LEN),
                thresholds=tuple(t if t == "0.5:0.95" else float(t) for t in thr))


def dense_setting(cfg):
    """CONFIG.VAL.VIDEO_MAP.DENSE validated (with the rest of VIDEO_MAP): the default of ``tubes(dense=)`` and, inherited like MAX_GAP, of
    ``tracks(dense=)``.  Kept out of ``video_map_settings``' dict: that one is the keyword arguments of the evaluators"""
    video_map_settings(cfg)
    return cfg.CONFIG.VAL.VIDEO_MAP.DENSE


def tube_nms_settings(cfg):
    """CONFIG.VAL.TUBE_NMS validated -> dict(iou, actors_iou), each None (off) or a float in [0, 1]; a bad value raises ValueError naming its key"""
    t = cfg.CONFIG.VAL.TUBE_NMS
    out = {}
    for key in ("IOU", "ACTORS_IOU"):
        v = t[key]
        if v is not None and (not isinstance(v, (int, float)) or isinstance(v, bool) or v != v or not 0.0 <= v <= 1.0):
            raise ValueError("CONFIG.VAL.TUBE_NMS.%s = %r: must be None or a number in [0, 1]" % (key, v))
        out[key.lower()] = None if v is None else float(v)
    return out


def crop_settings(cfg):
    """CONFIG.VAL.CROPS validated -> dict(size, scale, samples), the defaults of ``VideoDetections.crops``; a bad value raises ValueError naming its key"""
    c = cfg.CONFIG.VAL.CROPS

    def bad(key, why):
        raise ValueError("CONFIG.VAL.CROPS.%s = %r: %s" % (key, c[key], why))
    integer = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if not isinstance(c.SIZE, (list, tuple)) or len(c.SIZE) != 2 or not all(integer(v) and v >= 1 for v in c.SIZE):
        bad("SIZE", "must be two integers >= 1 (h, w)")
    if not isinstance(c.SCALE, (int, float)) or isinstance(c.SCALE, bool) or not 0.0 < c.SCALE < float("inf"):
        bad("SCALE", "must be a finite number > 0")
    if not integer(c.SAMPLES) or not 1 <= c.SAMPLES <= 4:
        bad("SAMPLES", "must be an integer in 1 .. 4")
    return dict(size=(int(c.SIZE[0]), int(c.SIZE[1])), scale=float(c.SCALE), samples=int(c.SAMPLES))


def detect_settings(cfg):
    """CONFIG.VAL.DETECT and CONFIG.VAL.GRAPHED validated -> dict(score_thr, topk, actor_thr, graphed); a bad value raises ValueError naming its key"""
    val = cfg.CONFIG.VAL
    d = val.DETECT

    def bad(key, value, why):
        raise ValueError("CONFIG.VAL.%s = %r: %s" % (key, value, why))
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    if not number(d.SCORE_THR) or not 0.0 <= d.SCORE_THR <= 1.0:
        bad("DETECT.SCORE_THR", d.SCORE_THR, "must be a number in [0, 1]")
    if not isinstance(d.TOPK, int) or isinstance(d.TOPK, bool) or d.TOPK < 1:
        bad("DETECT.TOPK", d.TOPK, "must be an integer >= 1")
    if not number(d.ACTOR_THR) or not 0.0 <= d.ACTOR_THR < 1.0:
        bad("DETECT.ACTOR_THR", d.ACTOR_THR, "must be a number in [0, 1)")
    if not isinstance(val.GRAPHED, bool):
        bad("GRAPHED", val.GRAPHED, "must be True or False")
    return dict(score_thr=float(d.SCORE_THR), topk=int(d.TOPK), actor_thr=float(d.ACTOR_THR), graphed=val.GRAPHED)


def actor_settings(cfg):
    """CONFIG.VAL.ACTORS validated, its None entries resolved -> dict(topk, link_iou, max_gap, min_len, window, label_thr); a bad value raises
    ValueError naming its key"""
    a = cfg.CONFIG.VAL.ACTORS
    vm, d = video_map_settings(cfg), detect_settings(cfg)

    def bad(key, why):
        raise ValueError("CONFIG.VAL.ACTORS.%s = %r: %s" % (key, a[key], why))
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    integer = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if a.LINK_IOU is not None and (not number(a.LINK_IOU) or not 0.0 <= a.LINK_IOU <= 1.0):
        bad("LINK_IOU", "must be None or a number in [0, 1]")
    if a.MAX_GAP is not None and (not integer(a.MAX_GAP) or a.MAX_GAP < 0):
        bad("MAX_GAP", "must be None or an integer >= 0")
    if a.MIN_LEN is not None and (not integer(a.MIN_LEN) or a.MIN_LEN < 1):
        bad("MIN_LEN", "must be None or an integer >= 1")
    if not integer(a.WINDOW) or a.WINDOW < 0:
        bad("WINDOW", "must be an integer >= 0")
    if a.LABEL_THR is not None and (not number(a.LABEL_THR) or not 0.0 <= a.LABEL_THR <= 1.0):
        bad("LABEL_THR", "must be None or a number in [0, 1]")
    if a.TOPK is not None and (not integer(a.TOPK) or a.TOPK < 1):
        bad("TOPK", "must be None or an integer >= 1")
    max_gap = int(vm["max_gap"] if a.MAX_GAP is None else a.MAX_GAP)
    topk = a.TOPK
    if topk is None:
        from . import lib
        topk = max(1, min(int(cfg.CONFIG.MODEL.QUERY_NUM), lib.query("tuber_tube_link_max_active") // (max_gap + 1)))
    return dict(topk=int(topk), link_iou=float(vm["link_iou"] if a.LINK_IOU is None else a.LINK_IOU), max_gap=max_gap,
                min_len=int(vm["min_len"] if a.MIN_LEN is None else a.MIN_LEN), window=int(a.WINDOW),
                label_thr=float(d["score_thr"] if a.LABEL_THR is None else a.LABEL_THR))


def load_cfg(path):
    cfg = get_cfg_defaults()
    cfg.merge_from_file(path)
    return cfg
