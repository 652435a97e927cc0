"""Every entry point include/tuber_hip.h declares is either named by a test under tests/ or listed in INDIRECT below with the test that
covers it and why it is not called directly.  A kernel exported without a test fails here, by name (CPU only: reads text files)."""
import glob
import os
import re

from tubelet_transformer_amd.lib import HEADER, header_prototypes

HERE = os.path.dirname(os.path.abspath(__file__))
RCCL = ("test_training_gpu.py", "test_one_rank_rccl_communicator_drives_the_ddp_step",
        "RCCL communicator calls: need ranks, driven through ddp.RcclComm by a one-rank communicator")

# entry point -> (test file, test function, reason it is covered indirectly)
INDIRECT = {
    "tuber_comm_version": RCCL,
    "tuber_comm_last_error": RCCL,
    "tuber_comm_etimedout": RCCL,
    "tuber_comm_unique_id": RCCL,
    "tuber_comm_init": RCCL,
    "tuber_comm_init_timeout": RCCL,
    "tuber_comm_count": RCCL,
    "tuber_comm_allreduce_sum": RCCL,
    "tuber_comm_allreduce_sum_multi": RCCL,
    "tuber_comm_destroy": RCCL,
    "tuber_adamw_segment": ("test_training_gpu.py", "test_fused_clip_adamw_matches_torch",
                            "launched by optim.FusedAdamW, which the test holds to torch.optim.AdamW + clip_grad_norm_"),
    "tuber_grad_norm_clip_coef": ("test_training_gpu.py", "test_fused_clip_adamw_matches_torch",
                                  "launched by optim.FusedAdamW, which the test holds to torch.nn.utils.clip_grad_norm_"),
    "tuber_clip_desc_bytes": ("test_input_pipeline.py", "test_gpu_clip_prepare_full_size",
                              "size query: input_pipeline checks its descriptor layout against it before tuber_clip_prepare"),
    "tuber_targets_pack_max": ("test_criterion_gpu.py", "test_padded_targets_refill_in_one_launch_equals_the_per_clip_copies",
                               "size query: PaddedTargets reads it to choose tuber_targets_pack"),
    "tuber_decoder_coop_ptrs_per_layer": ("test_training_gpu.py", "test_cooperative_decoder_launch_equals_the_launch_chain",
                                          "size query: the model builds the cooperative decoder's pointer table with it"),
    "tuber_gemm_tn_group_max": ("test_kernels_gpu.py", "test_gemm_tn_group_is_bit_identical_to_single_launches",
                                "size query: engine.TnGroup batches at most this many problems per tuber_gemm_tn_group launch"),
    "tuber_multi_reduce_entry_bytes": ("test_model_gpu.py", "test_deferred_weight_gradient_reductions_are_bit_identical",
                                       "size query: engine.DeferredReduce checks its entry layout against it"),
    "tuber_ln_bwd_dx_pays": ("test_kernels_gpu.py", "test_layernorm_backward_fused_into_the_linear_data_gradient",
                             "flag query: tape.py's choice between tuber_ln_bwd_dx and the two-launch path, both of which are tested"),
    "tuber_bn_bwd_fa_max_rows": ("test_kernels_gpu.py", "test_bn_bwd_one_launch_matches_finalize_plus_apply",
                                 "size query: the backbone's bound for tuber_bn_bwd_fa"),
    "tuber_gemm_nt_wsk96_set": ("test_kernels_gpu.py", "test_gemm_nt_wave_split_k",
                                "measurement switch (TUBER_NT_WSK96): selects between wave-split-K tile heights the test covers"),
}


def _test_sources():
    me = os.path.basename(__file__)
    return {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(HERE, "*.py")) if os.path.basename(p) != me}


def test_every_header_entry_point_has_a_test():
    names = [n for _, n, _ in header_prototypes(HEADER)]
    assert len(names) > 100, "header parse found only %d entry points" % len(names)
    text = "\n".join(_test_sources().values())
    named = {n for n in names if re.search(r"\b%s\b" % n, text)}
    uncovered = sorted(n for n in names if n not in named and n not in INDIRECT)
    assert not uncovered, ("entry points declared in include/tuber_hip.h that no test under tests/ names and that are not listed in "
                           "tests/test_entry_point_coverage.py INDIRECT: %s" % ", ".join(uncovered))


def test_indirect_table_names_existing_tests_and_declared_entry_points():
    names = {n for _, n, _ in header_prototypes(HEADER)}
    src = _test_sources()
    bad = []
    for name, (fname, test, reason) in sorted(INDIRECT.items()):
        if name not in names:
            bad.append("%s: not declared in the header any more (drop it from INDIRECT)" % name)
        if fname not in src or not re.search(r"^def %s\(" % re.escape(test), src[fname], flags=re.M):
            bad.append("%s: covering test %s::%s does not exist" % (name, fname, test))
        if not reason.strip():
            bad.append("%s: no reason given" % name)
    assert not bad, "\n".join(bad)
