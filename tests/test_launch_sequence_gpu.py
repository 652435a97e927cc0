"""The launch sequence of the default path, held to a recording: a change that is meant to leave the schedule alone (a refactor of
backbone.py / tape.py) must leave these files alone; one that changes what is launched regenerates them (scripts/launch_sequence.py)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_default_training_step_and_eval_forward_launch_the_recorded_sequence(dev, golden_dir, monkeypatch):
    """CSN-152 / AVA 2.1 at the smoke shape, first eager training step and first eval forward of a fresh model: entry point, every scalar
    argument and the NULL-ness of every pointer argument of every launch -- for a grouped weight-gradient launch every field of its host
    entries too, for the deferred reduction every entry of its device table -- equal tests/golden/launch_sequence_{train,eval}.txt line by line."""
    from tubelet_transformer_amd import ab
    assert ab.active() == [], "the recording is the default path's"
    monkeypatch.delenv("TUBER_EVAL_PRECISION", raising=False)
    spec = importlib.util.spec_from_file_location("launch_sequence", os.path.join(ROOT, "scripts", "launch_sequence.py"))
    ls = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ls)
    for case in ("train", "eval"):
        model, criterion = ls.fresh()
        fn = ls.step(model, criterion) if case == "train" else (lambda: ls.eval_forward(model, "fp32_stream"))
        want = open(os.path.join(golden_dir, "launch_sequence_%s.txt" % case)).read().splitlines()
        got = ls.record(fn)
        diff = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not diff and len(got) == len(want), (case, len(got), len(want), diff[:1] and (got[diff[0]], want[diff[0]]))
