"""TUBER_EVAL_PRECISION=fp32_class without a GPU: the mode's parsing and the C-ABI exports of its kernels (csrc/eval_f32.hip)."""
import importlib.util
import os

from tubelet_transformer_amd import ab, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp32_class_is_opt_in_and_read_at_call_time(monkeypatch):
    monkeypatch.delenv("TUBER_EVAL_PRECISION", raising=False)
    assert ab.eval_fp32_stream() and not ab.eval_class_f32()                 # default: fp32_stream, the branch on its bf16 path
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "fp32_stream")
    assert ab.eval_fp32_stream() and not ab.eval_class_f32()
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "fp32_class")
    assert ab.eval_fp32_stream() and ab.eval_class_f32()                      # fp32_class is fp32_stream plus the branch
    with ab.override("eval_bf16_stream"):
        assert not ab.eval_fp32_stream() and not ab.eval_class_f32()         # the bf16 streams switch wins
    with ab.override("eval_bf16_decoder"):
        assert ab.eval_class_f32()                                            # (tuber.py keeps the bf16 branch there: no hs32)
    monkeypatch.setenv("TUBER_EVAL_PRECISION", "bf16_stream")
    assert not ab.eval_fp32_stream() and not ab.eval_class_f32()


def test_header_declares_the_fp32_class_exports():
    protos = {name: args for _, name, args in lib.header_prototypes()}
    assert [t for t, _ in protos["tuber_attention_f32_mapped"]] == [
        "const float*", "const long*", "const float*", "const long*", "const float*", "const long*", "float*", "const long*",
        "int", "int", "int", "int", "float", "hipStream_t"]
    assert [t for t, _ in protos["tuber_layernorm_f32_rows"]] == [
        "const float*", "long", "const float*", "long", "const float*", "const float*", "float*", "long", "int", "int", "float", "hipStream_t"]
    # the existing fp32 exports keep their signatures
    assert [t for t, _ in protos["tuber_attention_f32"]] == [
        "const float*", "long", "const float*", "long", "const float*", "long", "float*", "long", "const void*", "int", "int", "int", "int", "float", "hipStream_t"]
    spec = importlib.util.spec_from_file_location("gen_header", os.path.join(ROOT, "tubelet_transformer_amd", "csrc", "gen_header.py"))
    gh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gh)
    defined = {n: f for f, _, n, _ in gh.prototypes()}
    for name in ("tuber_attention_f32_mapped", "tuber_layernorm_f32_rows"):
        assert defined[name] == "eval_f32.hip"
        assert "transformer_layers.py" in gh.DOC[name]                        # the reference op it replaces
