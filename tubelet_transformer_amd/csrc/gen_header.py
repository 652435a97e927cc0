"""Regenerate include/tuber_hip.h from the extern "C" definitions in csrc/*.hip.

The prototypes are extracted from the sources (so header and library cannot drift); the
per-function documentation -- what reference op each entry point replaces (file:line under
/root/reference) -- lives in DOC below.  Run:  python tubelet_transformer_amd/csrc/gen_header.py
"""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

DOC = {
    "tuber_gemm_nt_addproj": "packed attention in-projection with the positional embedding folded in: C = f(A).B^T + bias with f(A) = A + A2 for the output "
                             "columns [0, add_ncols) (q / k rows of in_proj_weight: with_pos_embed, models/transformer/transformer.py:150-159,215-240) and "
                             "f(A) = A for the v rows -- one GEMM instead of an add kernel and two GEMM launches. add_ncols % 128 == 0.",
    "tuber_bn_bwd_fa": "tuber_bn_bwd_finalize + tuber_bn_bwd_apply in ONE launch for short partial lists (layer3 / layer4 of the CSN body): every workgroup "
                       "derives the coefficients of its 128-channel strip from the R partial rows (fp64) and applies dx = cA*dz + cB*x + cC to its rows; "
                       "dgamma / dbeta accumulated by the first row chunk (NULL: frozen BatchNorm). autograd of nn.BatchNorm3d (ir_CSN_152.py:46,56,64,154).",
    "tuber_bn_bwd_fa_max_rows": "largest R tuber_bn_bwd_fa accepts.",
    "tuber_bn_frozen_affine_multi": "the FROZEN BatchNorm layers of a training-mode forward (nn.BatchNorm3d with module.training == False inside model.train(): "
                                    "F.batch_norm(training=False), models/backbones/ir_CSN_152.py:46,56,64,119,154) in ONE launch over a device table of "
                                    "{gamma, beta, running_mean, running_var, scale, shift, mean, invstd, cA, cB, cC, C} rows: scale / shift bit-identical to "
                                    "tuber_bn_eval_affine, mean = running_mean, invstd = 1 / sqrt(running_var + eps), and the backward coefficients cA = gamma * invstd, "
                                    "cB = cC = 0, so every backward kernel that takes (cA, cB, cC) runs unchanged. The running buffers are not written.",
    "tuber_bn_frozen_param_grads": "dgamma += sum dz * (x - running_mean) * invstd, dbeta += sum dz of a frozen BatchNorm whose affine parameters train (autograd of "
                                   "F.batch_norm(training=False), ir_CSN_152.py:46,56,64,119,154) from the partial rows (sum dz, sum dz*x) of the train-mode path: "
                                   "no count, no coefficient output.",
    "tuber_bn_bwd_fa_frozen": "tuber_bn_bwd_fa for a frozen BatchNorm: dx = gamma * invstd * dz in one launch (autograd of F.batch_norm(training=False), "
                              "ir_CSN_152.py:46,56,64,154); x is not an operand, the partial rows are read only for dgamma / dbeta (NULL: not at all).",
    "tuber_dwconv_tile_bwd_data_bn_frozen": "tuber_dwconv_tile_bwd_data_bn with a FROZEN bn3 above the depthwise conv (ir_CSN_152.py:53-56 with bn3.training == False): "
                                            "dc3 = gamma * invstd * dzu formed on load; the partial rows are read only for dgamma / dbeta (NULL: not at all).",
    "tuber_dwconv_tile_bwd_weight_bn_frozen": "tuber_dwconv_tile_bwd_weight_bn with a FROZEN bn3 (ir_CSN_152.py:53-56): takes no partial rows.",
    "tuber_dwconv_tile_bwd_both_bn_frozen": "tuber_dwconv_tile_bwd_both_bn with a FROZEN bn3 (ir_CSN_152.py:53-56): data and weight gradient of the depthwise conv in one "
                                            "launch with dc3 = gamma * invstd * dzu formed on load; dz and dgamma / dbeta bit-identical to tuber_dwconv_tile_bwd_data_bn_frozen.",
    "tuber_ln_bwd_dx": "tuber_layernorm_bwd (partial rows only) + the data-gradient tuber_gemm_nt of the linear layer in front of the LayerNorm in ONE launch: "
                       "autograd of tgt = norm(tgt + dropout(sublayer)) where the sublayer ends in out_proj / linear2 (models/transformer/transformer.py:160-167,229-247). "
                       "Every workgroup runs the LayerNorm backward of its 32 rows itself and multiplies the bf16 result from LDS with W on MFMA; the column-0 workgroups "
                       "store dx / dxd / the dgamma, dbeta partial rows ([tuber_ln_bwd_dx_blocks(M)][2E]) as the two-launch path does. dy2: a second gradient contribution (replaces "
                       "a tuber_axpby launch) or NULL; res: an existing gradient of the linear's input to add; cm / alpha: the ReLU / Dropout mask of that input.",
    "tuber_rows_dx2": "both data gradients of a packed attention in-projection with the positional embedding folded in (tuber_gemm_nt_addproj; "
                      "models/transformer/transformer.py:150-159,215-240) in ONE launch for few rows: dx = g.W over all N columns (+ res), dpos = g[:, :Nq].W[:Nq] "
                      "stored as a prefix of the same reduction. Replaces two tuber_gemm_nt launches per decoder in-projection.",
    "tuber_criterion_scale": "backward of tuber_criterion_loss's loss table in one launch: the stored per-layer gradients scaled by the incoming gradient of the [L][4] "
                             "losses (autograd of the weighted sum of loss terms, models/criterion.py:169-206 + train_tuber_ava.py loss weighting).",
    "tuber_weighted_sum": "sum_i a[i] w[i] on the device in a fixed order, or its backward gout * w: the weighted total of the loss terms "
                          "(pipelines/video_action_recognition.py:147) without ATen launches.",
    "tuber_ln_bwd_dx_blocks": "partial rows tuber_ln_bwd_dx writes for M rows (32 rows per block).",
    "tuber_ln_bwd_dx_pays": "1 where tape.py uses tuber_ln_bwd_dx instead of the two launches: M <= 64 rows at any width, or Kin <= 256 (measured; the encoder's linear2 loses).",
    "tuber_ln_bwd_dx_supported": "1 when tuber_ln_bwd_dx handles a LayerNorm of width E in front of a linear with Kin inputs (E = 256, Kin % 64 = 0).",
    "tuber_bn_bwd_fa_rows": "rows per workgroup tuber_bn_bwd_fa takes for (M, C): 64, 128 or 176 -- the grid that sits at or just under a multiple of the 256 CUs.",
    "tuber_bn_bwd_fa_rows_set": "test hook: rows per THREAD of tuber_bn_bwd_fa forced to 4, 8 or 11 (0 = the heuristic), so that tests cover every instantiation at every shape.",
    "tuber_class_error": "class_error of the matched queries of one decoder layer, on the device: 100 - exact-set accuracy (AVA, utils/misc.py:497-518 "
                         "via models/criterion.py:76-78) or top-1 accuracy (JHMDB, utils/misc.py:521-539 via criterion.py:258-260).",
    "tuber_targets_pack": "the padded [B, Tmax] target layout of one batch in ONE launch: boxes (column 0 = key-frame index dropped, models/detr/matcher.py:64, "
                          "models/criterion.py:106), labels (multi-hot rows for AVA, class ids for JHMDB) and the per-clip counts from B per-clip device tensors "
                          "whose pointers travel by value (HOST arrays boxes[B], labels[B], sizes[B]); zero padding included. Replaces the two memsets + two sliced "
                          "copies per clip the captured step issued before every replay.",
    "tuber_targets_pack_max": "largest B tuber_targets_pack accepts.",
    "tuber_decoder_coop_fwd": "the DETR decoder stack forward (TransformerDecoder.forward / TransformerDecoderLayer.forward_post, models/transformer/transformer.py:99-128,"
                              "218-249) as ONE cooperative launch: 16 workgroups on one XCD split every weight matrix by output columns, exchange the <= 32 x 256 activations "
                              "through that XCD's L2 and meet at 8 XCD-local barriers per layer. layer_ptrs: HOST array, tuber_decoder_coop_ptrs_per_layer() device pointers per "
                              "layer (6 bf16 weights: self in-proj, self out-proj, cross q rows, cross out-proj, linear1, linear2; their 6 fp32 biases; norm1 / norm2 / norm3 weight, "
                              "bias; the layer's packed memory projection [(memory + pos) W_k | memory W_v]; then the 21 tensors the launch chain saves for its backward: qkv, o1, lse1, "
                              "a1, y1, xhat1, rstd1, q, o2, lse2, a2, y2, xhat2, rstd2, h, f2, y3, xhat3, rstd3, xhatN, rstdN). layer_salts: HOST array, 6 dropout salts per layer. "
                              "sync: 4 zeroed 32-bit device words, left zero by a clean run; sync[2] != 0 afterwards = a barrier timed out (a workgroup was not co-resident): the kernel has "
                              "overwritten hs with NaN, so the step's loss / gradient norm are NaN and tuber_adamw_segment skips the update.",
    "tuber_block_out_fwd_f32": "tuber_block_out_fwd for the eval precision mode: y = relu(bn4(c4) + shortcut) (models/backbones/ir_CSN_152.py:84-90) with the residual "
                               "stream kept in fp32 between the bottlenecks -- reads the previous block's fp32 output, writes the bf16 GEMM operand AND the fp32 stream.",
    "tuber_layernorm_fwd_f32": "tuber_layernorm_fwd for the eval precision mode: LayerNorm(x + res) (models/transformer/transformer.py:160-167,229-247, post-norm) with the "
                               "residual stream in fp32 from LayerNorm to LayerNorm; writes the bf16 GEMM operand and (optionally) the fp32 stream.",
    "tuber_bn_eval_affine_multi": "tuber_bn_eval_affine (eval-mode nn.BatchNorm3d: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale; "
                                  "models/backbones/ir_CSN_152.py:46,56,64,154 under model.eval()) for every BatchNorm of the body in ONE launch over a device table of "
                                  "{gamma, beta, running_mean, running_var, scale, shift, C, unused} rows.",
    "tuber_gemm_nt_bn_out": "EVAL forward of a bottleneck's tail in ONE launch: conv4 on relu(bn3(c3)) + the eval-mode bn4 + the residual join + ReLU in the GEMM epilogue "
                            "(models/backbones/ir_CSN_152.py:62-64,84-90 under model.eval(): a BatchNorm is a constant affine map there, so the join does not wait for "
                            "statistics). Writes y as bf16 (next block's GEMM operand) and as fp32 (the residual stream of the eval precision mode); c4 never reaches HBM. "
                            "Replaces tuber_gemm_nt(amode 1) + tuber_block_out_fwd_f32 for identity blocks.",
    "tuber_block_out_fwd_mask": "tuber_block_out_fwd (y = relu(bn4(c4) + shortcut), models/backbones/ir_CSN_152.py:84-90) that also writes the ReLU mask of y as a bit field "
                                "([M][C / 8] bytes, bit e of byte (m, c / 8) = y[m][c + e] > 0) for the join backward (tuber_gemm_nt_join_mask).",
    "tuber_gemm_nt_join_mask": "tuber_gemm_nt_join (conv1 data gradient of bottleneck i+1 + the join backward of bottleneck i: autograd of ir_CSN_152.py:72,86-89) with the ReLU mask "
                               "[y > 0] read from the bit field of tuber_block_out_fwd_mask instead of y itself: identical results, M*N/8 bytes instead of 2*M*N.",
    "tuber_gemm_nt_join_ds_mask": "tuber_gemm_nt_join_ds with the ReLU mask read from the bit field of tuber_block_out_fwd_mask instead of y (identical results).",
    "tuber_gemm_nt_join_strided_mask": "tuber_gemm_nt_join_strided with the ReLU mask read from the bit field of tuber_block_out_fwd_mask / tuber_blockout_conv1_fwd_mask instead of y (identical results).",
    "tuber_blockout_conv1_fwd_mask": "tuber_blockout_conv1_fwd that also writes the ReLU mask of y as a bit field ([M][32] bytes) for the join backward across the stage boundary.",
    "tuber_linear_f32": "fp32 linear layer of the eval precision mode: y = act((x [+ add]) . W^T + bias) on the fp32 master weights -- the decoder's nn.Linear / packed "
                        "in-projections (models/transformer/transformer.py:218-249, with_pos_embed as the add operand) and the box / actor heads (models/tuber_ava.py:121-125,142; "
                        "MLP models/criterion.py:485-497) under model.eval().",
    "tuber_linear_f32_batched": "tuber_linear_f32 for nbatch weight sets over ONE input in one launch (set z: W + z * w_stride, bias + z * bias_stride, y + z * y_stride, strides in elements): "
                                "the memory-side K / V projections of all decoder layers (models/transformer/transformer.py:232-237), which do not depend on the decoder state.",
    "tuber_attention_f32": "fp32 multi-head attention core (head dimension 32) of the eval precision mode: the decoder's self- and cross-attention "
                           "(nn.MultiheadAttention, transformer.py:218-240) with fp32 scores, softmax and values.",
    "tuber_attention_f32_mapped": "tuber_attention_f32 with every operand read in place through a token map {ld,sL,s1,s2,B2} (tuber_attn_fwd's convention): "
                                  "the class branch of TUBER_EVAL_PRECISION=fp32_class run once per clip in fp32 -- its t- and s-attention (nn.MultiheadAttention "
                                  "self_attn_t / self_attn_s, transformer_layers.py:71-97) and the cross-attention of the decoder queries over the clip's "
                                  "encoded features (tuber_ava.py:127-141) with K / V at stride 0 over the decoder layer. No key padding mask. "
                                  "Lq, Lk <= 8: one thread per (sequence, query, head).",
    "tuber_layernorm_f32_rows": "fp32 LayerNorm(x + res) (nn.LayerNorm, transformer_layers.py:58-69, post-norm) with fp32 operands and output, each with its own "
                                "leading dimension, E = 256: the class branch's norm1_t / norm1_s (into the halves of the [t | s] concatenation) and norm2 "
                                "under TUBER_EVAL_PRECISION=fp32_class.",
    "tuber_flag_signal": "software ordering edge between two HIP streams, producer side: *flag += 1 (release, agent scope) once everything enqueued on the stream "
                         "before it has completed; capturable as the last node of a graph part. With tuber_flag_wait it replaces the hipEventRecord / "
                         "hipStreamWaitEvent pair between the backward stream and the gradient exchange's stream (DistributedDataParallel's reducer, "
                         "utils/model_utils.py:47-52): a pending cross-stream event wait slows every kernel of a launch-bound graph by ~1.3 us on this runtime.",
    "tuber_flag_wait": "consumer side: a one-wave kernel that polls *flag until it reaches `expect` (wrap-around safe), in front of the collective on the "
                       "exchange's stream; gives up after ~2 s, sets *err = 1 and lets the stream go on (the caller checks the word where it synchronises).",
    "tuber_decoder_coop_supported": "1 when tuber_decoder_coop_fwd takes this decoder (d_model 256, 8 heads, FFN 2048, batch * 8 == 16 attention units, batch * queries <= 32, <= 6 layers).",
    "tuber_decoder_coop_ptrs_per_layer": "device pointers per layer in tuber_decoder_coop_fwd's layer_ptrs (40).",
    "tuber_mask_resize": "F.interpolate(mask[None].float(), size=(h, w)).to(torch.bool)[0] (models/backbone_builder.py:85-86): nearest-neighbour resize of the "
                         "clip padding mask to the feature grid = the transformer's key-padding mask, ATen's source-index rule.",
    "tuber_gemm_nt_join": "conv1 data gradient of one bottleneck fused with the join backward of the bottleneck below it: dz = (A.B^T + R) * [Y > 0] "
                          "plus the BatchNorm-backward partial rows (sum dz, sum dz*Cm) per 64 output rows (tuber_gemm_nt_stat_rows) -- "
                          "tuber_gemm_nt(epi 0, +R) followed by tuber_block_out_bwd without dx reaching HBM (autograd of "
                          "models/backbones/ir_CSN_152.py:72,86-89 across a block boundary). Y = the lower block's output, Cm = its raw conv4 output; R may be NULL.",
    "tuber_gemm_nt_join_strided": "tuber_gemm_nt_join at a STAGE boundary: R is the data gradient of the upper stage's strided projection shortcut (one row per sampled "
                                  "position, n*To*Ho*Wo rows) and is added to the output rows (n, t, h, w) with t % st == h % ss == w % ss == 0 inside the epilogue -- replaces "
                                  "tuber_gemm_nt + tuber_rows_scatter_add + tuber_block_out_bwd (autograd of models/backbones/ir_CSN_152.py:72,86-89,155-161).",
    "tuber_gemm_nt_join_ds": "tuber_gemm_nt_join below a stage's FIRST block: Cd = the raw output of that block's projection shortcut, stat2 = the rows sum dz*cd of the "
                             "shortcut BatchNorm's backward (tuber_block_out_bwd's third statistics buffer). autograd of models/backbones/ir_CSN_152.py:86-89,155-161. "
                             "ldcd counts like the other epilogue leading dimensions: an odd one selects the bounds-checked instantiation (tuber_gemm_nt_join_ds_mask: TUBER_EINVAL).",
    "tuber_gemm_tn_group": "n <= tuber_gemm_tn_group_max() weight-gradient GEMMs (each exactly one tuber_gemm_tn: dW = G^T f(A) of a 1x1x1 conv, "
                           "autograd of models/backbones/ir_CSN_152.py:41,58,155-161) in ONE launch; args_host = HOST array of struct TuberGemmTNArgs "
                           "{const void* G; long ldg; const void* A; long lda; float* partial; float* out; int accumulate, M, N, K, amode, gather, "
                           "To, Ho, Wo, Ti, Hi, Wi, st, ss; const float* a_scale; const float* a_shift; float* bias_grad; const void* A2; long lda2;} (A2: optional addend, A := A + A2) with the meaning of the tuber_gemm_tn arguments. "
                           "Transpose-read kernel shapes only (N, K, ld multiples of 8, 64x64 tiles); several slabs need accumulate = 2 (the caller reduces them).",
    "tuber_gemm_nt_wsk_tile_rows": "rows per tile of the wave-split-K form tuber_gemm_nt takes for a plain-A (M, N, K): 0 (not taken), 64, or 96 (shapes whose "
                                   "64-row tiling has more workgroups than the chip has CUs while the 96-row one does not: the layer3 / layer4 long-K convs).",
    "tuber_gemm_nt_96_set": "EXPERIMENT hook (round 6): 0 switches the 96-row tiles of the regular tuber_gemm_nt pipeline off (64-row tiles for layer2's conv1 forward / conv4 data gradient).",
    "tuber_gemm_nt_wsk96_set": "EXPERIMENT hook: 0 switches the 96-row wave-split-K tiles of tuber_gemm_nt off (64-row tiles everywhere).",
    "tuber_gemm_tn_args_bytes": "sizeof(struct TuberGemmTNArgs) as compiled (host-side layout check).",
    "tuber_gemm_tn_group_max": "largest n tuber_gemm_tn_group accepts (the argument blocks travel by value in the kernel argument segment).",
    "tuber_comm_version": "RCCL bound at run time (dlopen librccl.so.1: the instance the host process already loaded, else ROCm's): its version code, "
                          "or < 0 when it cannot be loaded. Replaces the NCCL process group the reference's DistributedDataParallel wrapper uses "
                          "(utils/model_utils.py:43-52, pipelines/launch.py:44-49).",
    "tuber_comm_etimedout": "the (negative) return code of tuber_comm_init_timeout when a rank never reached the bootstrap (fatal for the job).",
    "tuber_comm_last_error": "message of the last failing tuber_comm_* call.",
    "tuber_comm_unique_id": "ncclGetUniqueId: rank 0 fills the 128-byte rendez-vous id (HOST memory) that every rank hands to tuber_comm_init "
                            "(shipped over any side channel: torch.distributed store, MPI, a file).",
    "tuber_comm_init": "ncclCommInitRank on HIP device `device` (collective over all `nranks` processes, one per GPU); *comm_out receives the communicator.",
    "tuber_comm_allreduce_sum": "in-place sum over all ranks of buf[0..count) (dtype 0 = fp32, 1 = bf16) enqueued on `stream` -- the gradient all-reduce DDP's "
                                "reducer issues per bucket (torch/nn/parallel/distributed.py via utils/model_utils.py:46-52), here on windows of the flat "
                                "gradient buffer with no bucket copies; stream-ordered, capturable into a hipGraph.",
    "tuber_comm_allreduce_sum_multi": "the same for n windows (HOST arrays ptrs[n], counts[n]) as ONE RCCL group.",
    "tuber_comm_destroy": "ncclCommDestroy.",
    "tuber_conv1_bwd_fused": "backward of the bottleneck's first pointwise conv through bn1, for the wide-activation stage (256-channel block input, P = 64: layer1), as ONE persistent kernel: "
                             "dc1 = cA*dz1 + cB*c1 + cC lives only in LDS; dx = dc1 . W1 + R -- with Cm given, the residual join of the identity block below: "
                             "dz = dx * [X > 0] plus the statistics rows of tuber_gemm_nt_join --; dW1 = dc1^T . X from the SAME X tile (one fp32 slab per workgroup). "
                             "With Cd (the raw output of the lower block's projection shortcut) the join is that of a stage's FIRST block: st2 receives the rows sum dz*cd of the shortcut BatchNorm's backward "
                             "(tuber_block_out_bwd's third statistics buffer). Replaces tuber_bn_bwd_apply + tuber_gemm_nt / tuber_gemm_nt_join (+ tuber_block_out_bwd) + tuber_gemm_tn. autograd of models/backbones/ir_CSN_152.py:72-74,84-90.",
    "tuber_conv1_bwd_slabs": "workgroups = fp32 weight-gradient slabs tuber_conv1_bwd_fused produces for M rows.",
    "tuber_conv1_bwd_supported": "1 for the (block-input channels, P) the fused conv1 backward is built for.",
    "tuber_blockout_conv1_fwd": "residual join of one bottleneck + the first pointwise conv of the NEXT one as ONE persistent kernel (256-channel block output: layer1, and layer1 -> layer2): "
                                "y = relu(bn4(c4) + shortcut) exactly as tuber_block_out_fwd writes it, kept in LDS per 64-row tile and multiplied with the next conv1 weight from there "
                                "(c1 + the partial statistics rows of tuber_gemm_nt epi 1) -- y is written once and not read back. models/backbones/ir_CSN_152.py:84-90 then :72-74.",
    "tuber_blockout_conv1_supported": "1 for the (block-output channels, next conv1 output channels) the fused forward kernel is built for.",
    "tuber_stem_conv_bwd_weight_bn": "tuber_stem_conv_bwd_weight with the stem BatchNorm's backward apply folded into its gradient operand: takes the masked gradient of "
                                     "bn's output (tuber_stem_pool_bwd), the raw conv output and cA / cB / cC of tuber_bn_bwd_finalize; G = bf16(cA*dz0 + cB*c0 + cC) is formed "
                                     "while the tile is parked in LDS. Replaces tuber_bn_bwd_apply + tuber_stem_conv_bwd_weight (autograd of ir_CSN_152.py:131-133).",
    "tuber_entry_conv_fwd": "layer1's first bottleneck: conv1 (64 -> 64) and the projection-shortcut conv (64 -> 256) from ONE pass over the block input "
                            "x [M, 64] (persistent 64-row tiles, both weight matrices resident in LDS), with the per-64-row statistics rows of both outputs "
                            "(what tuber_gemm_nt epi 1 writes; NULL in eval mode). models/backbones/ir_CSN_152.py:72-74 and :86-87.",
    "tuber_entry_conv_supported": "1 for the (block input channels, conv1 output channels, projection output channels) the fused entry kernel is built for.",
    "tuber_conv4_bwd_fused": "backward of the bottleneck's second pointwise conv through bn4, for the wide-activation stage (C4 = 256, P = 64: layer1), as ONE persistent kernel: "
                             "dc4 = cA*dz + cB*c4 + cC (bn4 backward apply; coefficients from tuber_bn_bwd_finalize) is formed per 64-row tile in LDS and feeds BOTH the data gradient "
                             "dz3 = (dc4 . W4) * [bn3(c3) > 0] (+ the per-tile statistics rows tuber_gemm_nt epi 2 writes) and the weight gradient dW4 = dc4^T . relu(bn3(c3)) "
                             "(one fp32 slab per workgroup: tuber_conv4_bwd_slabs(M)) -- dc4 never reaches HBM: 2 passes over the [M, C4] tensors instead of 5 "
                             "(tuber_bn_bwd_fa + tuber_gemm_nt + tuber_gemm_tn). autograd of models/backbones/ir_CSN_152.py:58-64,78-84. "
                             "sc3 = sh3 = NULL selects the projection-shortcut form (down_sample conv + BatchNorm of a stage's first block, ir_CSN_152.py:86-87): "
                             "c4 = the projection's output, c3 = the block input, w4t = the projection weight transposed; no mask, no activation, no statistics rows.",
    "tuber_conv4_bwd_slabs": "workgroups = fp32 weight-gradient slabs tuber_conv4_bwd_fused produces for M rows.",
    "tuber_conv4_bwd_supported": "1 for the (C4, P) the fused conv4 backward is built for.",
    "tuber_dwconv_tile_bwd_data_bn": "tuber_dwconv_tile_bwd_data with the BatchNorm backward of bn3 (autograd of nn.BatchNorm3d, ir_CSN_152.py:56,76-77) folded into its "
                                     "gradient operand: takes bn3's masked output gradient dzu, bn3's input xu (= c3) and the R <= 128 partial rows (sum dz, sum dz*x) "
                                     "instead of a finished dc3; every workgroup derives cA / cB / cC of its 64 channels (fp64) and forms dc3 = cA*dzu + cB*xu + cC "
                                     "in fp32 while staging. dgamma / dbeta of bn3 are accumulated (+=) unless NULL. Replaces tuber_bn_bwd_fa + tuber_dwconv_tile_bwd_data.",
    "tuber_dwconv_tile_bwd_both_bn": "data gradient AND weight gradient of one stride-1 depthwise conv (bn3's backward folded in) in ONE launch and ONE pass over the "
                                     "operands: both are sums over the same (p, p - off) position pairs, so the ring of dc3 staged for the data gradient also feeds "
                                     "dW[off] = sum_p relu(bn1(x))[p] * dc3[p - off] -- 4 tensor passes (read dzu, xu, x; write dz). dz / dgamma / dbeta bit-identical to "
                                     "tuber_dwconv_tile_bwd_data_bn, statistics rows and weight gradient equal up to fp32 summation order; partial = "
                                     "tuber_dwconv_tile_blocks(...) blocks of [27][C], reduced by the caller. The kernel addresses a plane with 32-bit byte offsets: planes of "
                                     "H * W * C * 2 >= 4 GiB are refused (TUBER_EINVAL), here and in the frozen form. autograd of models/backbones/ir_CSN_152.py:48-56,74-77.",
    "tuber_dwconv_tile_bwd_weight_bn": "tuber_dwconv_tile_bwd_weight with the same fold: the output-position gradient is formed from (dzu, xu, partial rows) on load.",
    "tuber_comm_init_timeout": "tuber_comm_init with a deadline: the bootstrap (a collective) runs on a helper thread and the call returns -3 with a message naming "
                               "the waiting rank when its peers have not arrived after timeout_ms -- a dead rank fails the job loudly instead of hanging it "
                               "(what torch.distributed's process-group timeout does for the reference, pipelines/launch.py:44-49). timeout_ms <= 0: no deadline.",
    "tuber_comm_count": "ncclCommCount / ncclCommUserRank of the communicator: the world size and rank RCCL itself sees (rank_out may be NULL).",
    "tuber_cast_bf16_f32_scale": "dst = float(src) * scale: expands a bf16-compressed, all-reduced gradient window back into the fp32 gradient buffer and averages it in the same pass.",
    "tuber_frames_resize": "PIL.Image.resize((nw, nh)) of every decoded frame (datasets/ava_frame.py:146-150; jhmdb_frame.py alike): Pillow's 8-bit two-pass "
                           "fixed-point bicubic (libImaging/Resample.c), packed RGB uint8 [nimg][H][W][3] -> [nimg][Ho][Wo][3], bit-exact.",
    "tuber_clip_prepare": "hflip + crop + ColorJitter + ToTensor/Normalize (datasets/video_transforms.py:69-85,20-66,333-369,308-322; pipeline "
                          "datasets/ava_frame.py:158-176) and the batch collate of utils/misc.py:279-282,367-425 in one pass: uint8 frames -> "
                          "fp32 [N][3][T][Hmax][Wmax] zero padded + bool mask [N][Hmax][Wmax]. One TuberClipDesc per clip (56 bytes: long long src_off; "
                          "int H, W, y1, x1, h, w, flip, jitter, hue, sat, val, pad).",
    "tuber_clip_desc_bytes": "sizeof(TuberClipDesc) as the library was compiled (host-side layout check).",
    "tuber_multi_reduce": "every deferred second-stage reduction of one backward pass in one launch: the weight-gradient launchers called with "
                          "accumulate = 2 (tuber_gemm_tn, tuber_dwconv_*_bwd_weight, tuber_colsum, tuber_layernorm_bwd) leave their partials in place; "
                          "table = MultiReduceEntry[] {const float* P; float* out; long n, stride; int S, mode, C, next}: out[j] += sum_s P[s*stride+j] "
                          "(mode 0 / 2: per element / per float4, s ascending; mode 1: 32-way tree; C > 0: depthwise [S][27][C] -> [C][27]; next: chained contribution to the same out); blk = int2[] (head entry, block in entry), "
                          "1024 / 4096 / 32 elements per block in mode 0 / 2 / 1. Same summation order as the immediate kernels.",
    "tuber_multi_reduce_entry_bytes": "sizeof(MultiReduceEntry) as compiled (host-side layout check).",
    "tuber_temporal_max_fwd": "nn.MaxPool3d((T,1,1)) over the T frames of the backbone features, TEMPORAL_DS_STRATEGY 'max' (models/backbone_builder.py:45-47,73): "
                              "rows (b,t,p) of E bf16 -> rows (b,p) + the uint8 index of the first maximal frame (arg may be NULL in eval).",
    "tuber_temporal_max_bwd": "backward of tuber_temporal_max_fwd: the gradient goes to the frame that held the maximum, zeros elsewhere.",
    "tuber_gemm_nt": "C[M,N] = f(A)[M,K] . B[N,K]^T on MFMA bf16. Replaces every nn.Conv3d(k=1) of the CSN bottlenecks "
                     "(models/backbones/ir_CSN_152.py:41,58,155-161), input_proj/class_proj (models/tuber_ava.py:57-58) and every "
                     "nn.Linear / packed in-projection (models/transformer/transformer.py:159-165,227-245; transformer_layers.py:81-94; "
                     "tuber_ava.py:65-71), plus their data gradients (B = W^T). amode 1 fuses relu(x*a_scale[k]+a_shift[k]) "
                     "(BatchNorm apply, ir_CSN_152.py:72-79) into the A load; gather=1 reads A rows through the strided "
                     "(n,t*st,h*ss,w*ss) map of the down_sample conv (:155-161). epi 0: +bias, +R, ReLU, bf16|fp32 out; "
                     "epi 1: bf16 out + per-column partial (sum, sum^2) rows for training-mode BatchNorm; epi 2: out = acc*[Cm*m_scale+m_shift>0] "
                     "+ partial (sum dz, sum dz*Cm) rows for BatchNorm backward (stat rows optional: with m_scale NULL it is the ReLU / ReLU+Dropout "
                     "backward mask from the saved activation). Accumulators are scaled by alpha first; epi 0 can end with Dropout(drop_p) "
                     "keyed by (seed, salt, m*N+n) -- FFN linear1 (transformer.py:160-162). K % 64 == 0. "
                     "LAYOUT CONTRACT of this entry point and its siblings (tuber_gemm_nt_addproj, _join*, _bn_out): lda / ldb / lda2 are multiples of 8 (else TUBER_EINVAL) "
                     "and A / B / A2 start on a 16-byte boundary -- the main loop loads 16 bytes; the base pointers are the caller's responsibility and are NOT checked. "
                     "The epilogue's tensors (C, R, Cm, Y, Cd) take any leading dimension >= N: with N a multiple of the tile width and every one of those leading dimensions "
                     "a multiple of 8 the FULL instantiation (16-byte accesses) runs, otherwise the bounds-checked one (element accesses), with bit-identical results; "
                     "a tensor whose leading dimension is a multiple of 8 must start on a 16-byte boundary. Nothing outside rows [0, M) x columns [0, N) of an output "
                     "and nothing outside rows x [0, K) / [0, N) of an operand is touched. The bit-field joins and tuber_gemm_nt_bn_out are built FULL only (TUBER_EINVAL otherwise).",
    "tuber_gemm_nt_cfg": "tile configuration tuber_gemm_nt uses for (M,N,K): 13 = 64x64 (two-tile prefetch), 7 = 64x128, 0 = 128x128 (plain epilogue only); "
                         "the forced configuration while tuber_gemm_nt_set_cfg holds. What is launched after the form and epilogue rules: tuber_gemm_nt_plan.",
    "tuber_gemm_nt_plan": "what tuber_gemm_nt and its siblings launch for (M, N, K, amode, epi, gather, out_f32), packed as form * 1000000 + tile rows * 1000 + tile "
                          "columns: form 0 = the shared-tile pipeline (128x128, 64x128, 64x64), 1 = wave split-K (64x64, 96x64), 2 = 96x64 tiles on the regular "
                          "pipeline; TUBER_EINVAL where the (amode, epi) combination is not built for the shape. aligned: every leading dimension of the epilogue's "
                          "tensors is a multiple of 8 (ldc = N). Reads the same decision the launchers take (tile hooks included); host only.",
    "tuber_gemm_tn_tile": "output tile edge of the transpose-read weight-gradient kernel for (M, N, K): 128 (mid-M backbone shapes, N and K multiples of 128) or 64.",
    "tuber_gemm_nt_has_cfg": "1 when tuber_gemm_nt_set_cfg(cfg) names a tile configuration this library was built with.",
    "tuber_gemm_nt_stat_rows": "rows of partial statistics tuber_gemm_nt(epi 1|2) writes for (M,N).",
    "tuber_gemm_tn": "dW[N,K] (+)= sum_m G[m,N]^T . f(A)[m,K]: weight gradient of the same convs / linears (autograd of the ops above); "
                     "split over M into fp32 slabs `partial` [tuber_gemm_tn_slabs][N][K], then reduced deterministically. "
                     "LAYOUT CONTRACT: ldg / lda are multiples of 4 and >= ceil4(N) / ceil4(K) (else TUBER_EINVAL). N, K, ldg, lda all multiples of 8: the transpose-read kernels, "
                     "16-byte loads, G / A (and partial / out) on 16-byte boundaries. Otherwise the in-register-transpose kernel: 8-byte loads, G / A on 8-byte boundaries; it reads "
                     "whole 4-column groups, i.e. up to ceil4(N) / ceil4(K) columns of a row, and the values in those pad columns (anything, NaN included) only reach output "
                     "rows / columns that are never stored. Base pointers are NOT checked. partial / out / bias_grad are dense.",
    "tuber_gemm_tn_fuses_bias": "can tuber_gemm_tn also produce the bias gradient for this shape: 0 no; 1 yes, accumulated into bias_grad[N] directly (single slab); 2 yes, bias_grad receives one partial row per slab ([tuber_gemm_tn_slabs][N], reduced by the caller).",
    "tuber_gemm_tn_slabs": "number of slabs (size of `partial` / (N*K)) tuber_gemm_tn uses.",
    "tuber_dwconv_fwd": "depthwise Conv3d(C,C,3,groups=C,stride=(st,ss,ss),padding=1) on NDHWC bf16, ResNeXtBottleneck.conv3 "
                        "(ir_CSN_152.py:48-51) with relu(bn1(.)) fused on load (sc/sh may be NULL) and bn3 partial statistics on store.",
    "tuber_dwconv_bwd_data": "input gradient of conv3 fused with the backward of relu(bn1(.)): dz = da*[x*sc+sh>0] + partial (sum dz, sum dz*x).",
    "tuber_dwconv_bwd_weight": "weight gradient of conv3 ([C][27] fp32), activation relu(bn1(x)) recomputed on load.",
    "tuber_dwconv_fwd_stat_rows": "partial-stat rows written by tuber_dwconv_fwd.",
    "tuber_dwconv_bwd_data_stat_rows": "partial-stat rows written by tuber_dwconv_bwd_data.",
    "tuber_dwconv_bwd_weight_blocks": "blocks (size of `partial` / (27*C)) used by tuber_dwconv_bwd_weight.",
    "tuber_dwconv_tile_fwd_bn": "tuber_bn_finalize + tuber_dwconv_tile_fwd in ONE launch: the training-mode BatchNorm in front of conv3 (bn1, ir_CSN_152.py:46-51) is "
                                "finalised inside the conv -- every workgroup derives scale / shift of its 64 channels from the producing conv's R partial rows "
                                "(pst0 = sum x, pst1 = sum x^2 over `count` rows; fp64 sums, the arithmetic of tuber_bn_finalize expression for expression), the first "
                                "workgroup of each channel group writes scale / shift / mean / invstd [C] and updates rmean / rvar / nbt (NULL: none). Other arguments as tuber_dwconv_tile_fwd.",
    "tuber_dwconv_tile_fwd_bn_ex": "tuber_dwconv_tile_fwd_bn with the momentum contract of tuber_bn_finalize_ex: the module's momentum as given, or (momentum < 0) "
                                   "the cumulative average of nn.BatchNorm3d(momentum=None) with nbt read, not written (tuber_bn_count_advance). "
                                   "reference: ir_CSN_152.py:46-51 under torch.optim.swa_utils.update_bn.",
    "tuber_dwconv_tile_fwd": "stride-1 conv3 (ir_CSN_152.py:48-51) with the input planes staged once per workgroup in an LDS ring (activated on the way in): "
                             "same contract as tuber_dwconv_fwd for st = ss = 1; partial-stat rows = tuber_dwconv_tile_blocks.",
    "tuber_dwconv_tile_bwd_data": "LDS-staged data gradient of the stride-1 conv3, fused with the backward of relu(bn1(.)) like tuber_dwconv_bwd_data.",
    "tuber_dwconv_tile_bwd_weight": "LDS-staged weight gradient of the stride-1 conv3 (activation recomputed while staging).",
    "tuber_dwconv_tile_blocks": "workgroups along x of the LDS-staged depthwise kernels = partial-stat rows / weight-gradient partial blocks.",
    "tuber_dwconv_tile_wgrad_blocks": "partial blocks (size of `partial` / (27*C)) of tuber_dwconv_tile_bwd_weight.",
    "tuber_dw_wgrad_reduce": "dw[c][tap] (+)= sum_r partial[r][tap][c]: second stage of the depthwise weight gradient.",
    "tuber_bn_finalize": "training-mode nn.BatchNorm3d(eps=1e-3, momentum=0.1) statistics (ir_CSN_152.py:15-16,46,56,64,119,154): partial rows -> "
                         "mean/invstd, scale=gamma*invstd, shift=beta-mean*scale, running_mean/var (unbiased) and num_batches_tracked update.",
    "tuber_bn_finalize_ex": "tuber_bn_finalize with the module's momentum as given (nn.BatchNorm3d.momentum, ir_CSN_152.py:15-16,46,56,64,119,154; "
                            "running = (1 - m) * running + m * batch, num_batches_tracked += 1). momentum < 0 selects the cumulative average of "
                            "momentum=None (torch.nn.modules.batchnorm._BatchNorm.forward): m = 1 / (n + 1) with n = *num_batches_tracked read on the device, "
                            "which this launch leaves unchanged so that every workgroup sees the same n -- tuber_bn_count_advance increments it after the forward.",
    "tuber_bn_count_advance": "num_batches_tracked += 1 (the `self.num_batches_tracked.add_(1)` of _BatchNorm.forward under momentum=None) for every BatchNorm "
                              "of a DEVICE table of n int64 counter addresses, in ONE launch: the layers finalised in cumulative mode by tuber_bn_finalize_ex / "
                              "tuber_dwconv_tile_fwd_bn_ex during the forward.",
    "tuber_stat_rows_reduce": "first stage for long partial-statistics lists (R > 512 rows: layer1): [R][C] x2 -> [tuber_stat_rows_reduced(R)][C] x2.",
    "tuber_stat_rows_reduced": "rows left by tuber_stat_rows_reduce (R itself when no first stage is needed).",
    "tuber_bn_eval_affine": "eval-mode BatchNorm3d folded to scale/shift from the running statistics.",
    "tuber_bn_bwd_finalize": "BatchNorm backward coefficients: dx = cA*dz + cB*x + cC, dgamma = sum dz*xhat, dbeta = sum dz.",
    "tuber_bn_bwd_apply": "dx = cA*dz + cB*x + cC (BatchNorm backward apply), bf16 [M,C].",
    "tuber_block_out_fwd": "bottleneck join y = relu(bn4(c4) + shortcut) (ir_CSN_152.py:81-90); shortcut = res or bn_ds(res) when rs/rh given.",
    "tuber_block_out_bwd": "backward of the join: dz = dy*[y>0] and the partial statistics of bn4 (and of the down_sample BN).",
    "tuber_rowblock_count": "partial-stat rows written by the row-blocked reduce kernels for M rows.",
    "tuber_layernorm_fwd": "y = LayerNorm(Dropout_p(x) (+ res)) over E in {256, 2048}, eps 1e-5 (nn.LayerNorm, transformer.py:163-167,229-247,116-123; "
                           "transformer_layers.py:84,91,96,437-445); saves xhat (bf16) and rstd for backward.",
    "tuber_layernorm_bwd": "backward of tuber_layernorm_fwd: dx (gradient of res), dxd (gradient of x through the regenerated dropout mask) and dgamma/dbeta via block partials.",
    "tuber_layernorm_bwd_blocks": "blocks used by tuber_layernorm_bwd (partial = 2*blocks*E floats).",
    "tuber_reduce_rows": "out[c] (+)= sum_r P[r][c].",
    "tuber_colsum_blocks": "row blocks (size of `partial` / C) used by tuber_colsum.",
    "tuber_colsum": "bias gradient: out[c] (+)= sum_m g[m][c] for bf16 g.",
    "tuber_gemm_nt_set_cfg": "tuning hook: force tile configuration cfg for every later tuber_gemm_nt (-1 = automatic choice).",
    "tuber_stem_conv_fwd": "stem Conv3d(3,64,(3,7,7),s=(1,2,2),p=(1,3,3)) (ir_CSN_152.py:109-115) as an implicit MFMA GEMM from the fp32 NCDHW clip to NDHWC bf16, "
                           "with the partial statistics of the following BatchNorm; Wp = tuber_stem_pack_weight(conv1.weight).",
    "tuber_stem_conv_bwd_weight": "weight gradient of the stem conv ([64][441] fp32) as an implicit MFMA GEMM (no patch matrix in HBM).",
    "tuber_stem_conv_blocks": "persistent grid size of the stem conv forward = its partial-stat rows.",
    "tuber_stem_conv_wgrad_blocks": "workgroups (= [512][64] fp32 partial slabs) of tuber_stem_conv_bwd_weight.",
    "tuber_stem_pack_weight": "conv1.weight [64][441] fp32 -> [64][512] bf16 with k' = (c,kt,kh)*8 + kw (zero padded).",
    "tuber_stem_pool_fwd": "relu(bn1(.)) + MaxPool3d((1,3,3),s=(1,2,2),p=(0,1,1)) (ir_CSN_152.py:119-122) on NDHWC bf16, C=64; saves the argmax tap.",
    "tuber_stem_pool_bwd": "backward of the pool + relu(bn1(.)): dz and the BN-backward partial statistics.",
    "tuber_stem_pool_bwd_stat_rows": "partial-stat rows written by tuber_stem_pool_bwd.",
    "tuber_attn_fwd": "softmax(scale*QK^T + key_padding_mask)[dropout] V for 32-wide heads, operands read in place through strided token maps "
                      "{ld,sL,s1,s2,B2}: row(l,b) = l*sL + (b/B2)*s1 + (b%B2)*s2. Core of nn.MultiheadAttention "
                      "(transformer.py:159,227,237; tuber_ava.py:138; transformer_layers.py:81,88) and of the hand-rolled MHA (:156-167,306-366).",
    "tuber_attn_bwd": "gradients dQ, dK, dV of tuber_attn_fwd (P recomputed from the saved log-sum-exp).",
    "tuber_attn_wide_fwd": "single-query, 256-wide-head attention of the LSTR pooling decoder (TEMPORAL_DS_STRATEGY decode; "
                           "backbone_builder.py:74-78, transformer_layers.py:156-167,306-366): q [NQ,2048], kv [rows,4096]=[k|v], T<=8 slots per pixel.",
    "tuber_attn_wide_bwd": "gradients dq [NQ,2048] and dkv [rows,4096] of tuber_attn_wide_fwd.",
    "tuber_lsap": "rectangular linear sum assignment on HOST doubles; restates scipy.optimize.linear_sum_assignment (call sites "
                  "models/detr/matcher.py:80, matcher_ucf.py:82) incl. its tie-breaking.",
    "tuber_lsap_device": "the same assignment (scipy.optimize.linear_sum_assignment semantics incl. tie-breaking; matcher.py:80, matcher_ucf.py:82) for all "
                         "(decoder layer, clip) problems at once ON THE DEVICE, one thread per problem: match[l][b][t] = query of target t.",
    "tuber_grad_norm_clip_coef": "global L2 norm of the flat gradient buffer and the clip coefficient min(1, max_norm/(norm+1e-6)), left on the device: "
                                 "torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1) (utils/video_action_recognition.py:153).  A non-finite norm "
                                 "yields coefficient -1 = skip the update and leaves the step count alone: the reference stops BEFORE optimizer.step() on a "
                                 "non-finite loss (video_action_recognition.py:195-198).",
    "tuber_adamw_segment": "AdamW update (torch.optim.AdamW semantics: decoupled decay, bias correction) of one contiguous flat segment with the "
                           "clip coefficient applied to the gradient on the fly (video_action_recognition.py:154; groups train_tuber_ava.py:41-58).",
    "tuber_weight_average": "weight averaging of the flat fp32 parameter buffer in one streaming pass: avg[i] += w * (p[i] - avg[i]) (an element with p == avg keeps its "
                            "bits; w == 1 stores p exactly). mode 0 (ema) restates timm's ModelEmaV2, w = 1 - decay, with warmup w = 1 - min(decay, (1 + n) / (10 + n)); "
                            "mode 1 (swa) the default avg_fn of torch.optim.swa_utils.AveragedModel, w = 1 / n; n = *n_avg + 1, w formed in fp64 and rounded once. "
                            "table = DEVICE {float decay; int mode, warmup, start, period}. With clip (norm_out of tuber_grad_norm_clip_coef) a step AdamW skipped "
                            "(clip[1] < 0) is not averaged; with step_ptr (the AdamW step count t) the update happens iff t >= start and (t - start) % period == 0; "
                            "a NULL pointer drops its test. *n_avg advances by one iff the update was applied (a one-thread launch behind the pass). The reference "
                            "trains without weight averaging (the epoch loop of train_tuber_ava.py:73-84); the grid is capped at 2048 workgroups of 256 threads x 4 elements.",
    "tuber_tensor_stats": "the step monitor: one 8-float row per parameter tensor over the flat fp32 buffers -- {sum g^2, max |g|, non-finite g, g == 0, sum p^2, max |p|, "
                          "non-finite p, sum u^2} with sums and maxima over the finite elements, counts as floats (saturated at 2^24) and u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps), "
                          "the AdamW direction of tuber_adamw_segment before lr and without the decay term (bc = 1 - beta^t formed in fp64 from the fp32 beta, rounded once; "
                          "m or v NULL: 0). What p.grad.norm() / p.norm() per parameter would cost ~700 launches and a host sync for; the reference logs the loss terms only "
                          "(utils/video_action_recognition.py:182-220). Deterministic, no atomics, three launches: 256 threads per chunk of <= tuber_tensor_stats_chunk() elements "
                          "of one tensor -> partial[n_chunks][8]; a wave per tensor adds its chunks in a fixed order; one thread does the bookkeeping. "
                          "tensors = DEVICE TensorStatsTensor[] {int chunk0, nchunks; float beta1, beta2, eps;}, chunks = DEVICE TensorStatsChunk[] {long off; int n, tensor;} "
                          "(off = first element, 64-element aligned window start + a multiple of the chunk). state = DEVICE int[4] {every, history, bad_count, bad_step}. "
                          "With step_ptr (the AdamW step count t) and clip (norm_out of tuber_grad_norm_clip_coef): a good step records iff t % every == 0, into "
                          "ring[(t / every) % history][n_tensors][8] with row_step[slot] = t, row_norm[slot] = {clip[0], clip[1]}, otherwise every workgroup returns at once; a step "
                          "AdamW skipped (clip[1] < 0) writes bad[n_tensors][8] and bad_step = t only while bad_count == 0 (keep-first) and always advances bad_count. "
                          "NULL clip: a good step; NULL step_ptr: no cadence, ring slot 0, no bias correction. g, p, m, v 16-byte aligned.",
    "tuber_frame_match": "validation frame-mAP on the device, matching step: for every frame f (rows [det_off[f], det_off[f + 1]) of det_box [N][4] fp32 xyxy / det_score "
                         "[N][C] fp32; rows [gt_off[f], gt_off[f + 1]) of gt_box [G][4] fp64 / gt_lab [G][C] bytes; det_off, gt_off DEVICE int[F + 1]) and every class c the "
                         "greedy matching of the PASCAL evaluator the reference drives (evaluates/evaluate_ava.py:150, evaluates/utils/per_image_evaluation.py:354-366,445-449): "
                         "valid detections by descending score[:, c] (equal scores by ascending row: a defined rule, the reference inherits numpy's unstable sort), j = first arg-max of "
                         "the fp64 IoU over the frame's ground-truth boxes labelled c, true positive iff iou[j] >= iou_thr and j not taken. flags [N][C] bytes: 1 true positive, 0 false "
                         "positive, 2 not counted (x1 >= x2 or y1 >= y2; class_mask[c] == 0, NULL mask: all classes), 3 a frame beyond the bounds (nothing decided). Sizes no frame list can "
                         "meet (N > F * max_dets, G > F * max_gt), bad sizes or pointers: negative, nothing launched. One workgroup per frame, lanes over classes, the n x g IoU table in LDS.",
    "tuber_frame_match_top1": "validation frame-mAP on the device, matching step under the JHMDB / UCF101-24 counting rule (evaluates/evaluate_ucf.py:109-126 over the same PASCAL "
                              "matching, evaluates/utils/per_image_evaluation.py:354-366,445-449): a row of det_prob [N][C + 1] fp32 (columns [0, C) the classes, column C no-object) is ONE "
                              "detection, of its arg-max column a (np.argmax: the first maximum, a NaN counting as one) with score det_prob[r][a]. det_cls [N] out: a. det_flag [N] bytes out: "
                              "2 not counted (a == C; x1 >= x2 or y1 >= y2; frame_skip[f] != 0, frame_skip [F] bytes or NULL: the frames a ground-truth box under 10 px^2 excludes, "
                              "evaluate_ucf.py:60-62), else with (bj, bv) the first arg-max of the fp64 IoU over the frame's ground-truth rows with gt_cls [G] == a (0-based; a class outside "
                              "[0, C) matches nothing): 1 iff bv >= iou_thr and no other counted row of the frame with the same bj and bv >= iou_thr ranks higher (score descending, equal scores by "
                              "ascending row, NaN last) -- the sequential greedy matching in closed form -- else 0; no candidate: 0. Offsets (DEVICE int[F + 1]), bounds and refusals as "
                              "tuber_frame_match; a frame beyond the bounds gets det_flag 3 and det_cls -1. One wave per frame, one lane per detection, four frames per workgroup, no LDS, no atomics.",
    "tuber_frame_match_max_dets": "detections per frame tuber_frame_match takes (64).",
    "tuber_frame_match_max_gt": "ground-truth boxes per frame tuber_frame_match takes (32).",
    "tuber_ranked_ap": "validation frame-mAP on the device, ranking step: VOC average precision per class (area under the monotone precision envelope, summed where recall changes; "
                       "evaluates/utils/metrics.py compute_precision_recall + compute_average_precision) from flags_ranked [C][N] bytes in rank order (1 true positive, 0 false positive, "
                       "anything else counts nowhere) and n_gt [C]: ap [C] fp64, NaN where n_gt <= 0, 0.0 where nothing is counted; n_tp [C] true positives (NULL: not wanted). One workgroup "
                       "per class, fp64, two sweeps over 4096-entry chunks with carries in a fixed order: no atomics, the same bits every run. N == 0 is legal.",
    "tuber_tube_link": "video-mAP on the device, linking step (evaluation.VideoMAP.link: the definition; the reference ships the frame-level evaluator "
                       "evaluates/evaluate_ucf.py only): det_box [N][4] fp32 xyxy / det_prob [N][C + 1] fp32 in layout order (video, slot, store order), slot_off DEVICE "
                       "int[S + 1] rows per slot, video_off DEVICE int[V + 1] slots per video. A row counts as one detection of its arg-max column (np.argmax; not when that "
                       "is no-object, the box has x1 >= x2 or y1 >= y2, or the probability is NaN). Per (video, class), slots ascending: the tubes whose last detection is "
                       "at most max_gap + 1 slots back are visited by descending mean score (fp64 sum of the fp32 scores / count), equal means by ascending head; each takes, "
                       "among the slot's unclaimed rows of the class whose fp64 IoU with its last box is >= link_iou, the highest score (equal scores by ascending row); rows "
                       "left over start tubes. Out: row_cls [N] the arg-max column, row_head [N] the layout row of the tube's first detection (-1: not counted), and at head "
                       "rows tube_score (fp64 mean), tube_len, tube_last (last slot). max_rows: the largest number of rows in a slot (the caller knows it). max_rows > "
                       "tuber_frame_match_max_dets(), max_rows * (max_gap + 1) > tuber_tube_link_max_active(), N > S * max_rows, bad sizes or pointers: negative, nothing "
                       "launched. One wave per (video, class): a lane holds one active tube and one row of the slot; no LDS, no atomics.",
    "tuber_tube_link_ranked": "tuber_tube_link over ranked detections (detect.Detections / video.VideoDetections; evaluation.link_rows: the definition): a row's class and "
                              "score are det_label [N] int (0-based; negative or >= C: the row is not counted) and det_score [N] fp32 instead of the arg-max of a "
                              "[N][C + 1] row. Arguments, outputs, bounds, negative codes, the wave-per-(video, class) walk and the fp64 sequential mean are "
                              "tuber_tube_link's, whose kernel body it shares; row_cls: the label, C for a row that is not counted. A padded [S][K] detection store "
                              "is passed as it is: slot_off = arange(S + 1) * K, the rows behind a key's count carry label -1.",
    "tuber_video_clips": "the clips of B key frames gathered from ONE resident video (datasets/ava_frame.py:43,143-150: every FRAME_RATE-th frame from "
                         "max(key - T//2 * rate, 0), the indices clipped; datasets/jhmdb_frame.py:201-213; then ToTensor + Normalize, "
                         "datasets/video_transforms.py:308-322): out[b][c][t][y][x] = lut[c][frames[clamp(index[b][t], 0, nframes - 1)][y1 + y][x1 + x][c]]. frames uint8 "
                         "[nframes][H][W][3] packed at any byte alignment, index DEVICE int[B][T] (clamped by the kernel), (y1, x1, h, w) the window taken of every "
                         "frame (Resize_Custom, video_transforms.py:210-227), lut fp32 [3][256], out fp32 [B][3][T][h][w]. 16-byte stores and dword loads from the "
                         "enclosing aligned window when w % 4 == 0, byte loads and scalar stores otherwise; the table in LDS. A null pointer, a non-positive size "
                         "or a window outside H x W: negative, nothing launched.",
    "tuber_video_clips_ring": "tuber_video_clips over a ring of the last R frames (video.VideoStream), the frame-index rule evaluated in the kernel: no index table is "
                              "built or uploaded. ring uint8 [R + 1][H][W][3] packed at any byte alignment: frame f sits in slot f % R, and frame 0 in the fixed slot R "
                              "as well (the jhmdb rule pads a short clip at the END of a video with frame 0, datasets/jhmdb_frame.py:205-208). Key b of the batch is "
                              "first_key + min(b, n_keys - 1) * key_step (the last batch repeats its last key); rule 0 ava (datasets/ava_frame.py:43,143-145), 1 jhmdb "
                              "(datasets/jhmdb_frame.py:201-208), 2 edge: video.clip_indices restated in closed form; n_total the video's frame count, < 0 while it is "
                              "not known (no end clamp). Window, lut, out and the load / store body are tuber_video_clips', the buffer bounds those of the R + 1 slots. "
                              "The caller guarantees that the ring holds every frame a key needs. A null pointer, a non-positive size, R < 1, an unknown rule, a "
                              "negative key or a window outside H x W: negative, nothing launched.",
    "tuber_tube_link_stream": "tuber_tube_link_ranked for ONE video whose slots arrive in pieces (evaluation.TubeLinker: the definition; video.VideoStream): links the S "
                              "new slots with the ordinals slot_base .. slot_base + S - 1, K rows each (det_box [S * K][4], det_label / det_score [S * K]; rows behind a "
                              "key's count carry label -1). state: caller-owned, tuber_tube_link_state_bytes(C) bytes, 16-byte aligned, all zero = no tubes: per (class, "
                              "lane) what a lane of the link kernel holds (valid, last box, fp64 sum, count, last ordinal, head), loaded before the walk and stored after "
                              "it with plain vector stores. Out, per row: row_head the GLOBAL row (ordinal * K + position) of the tube's first detection, row_score the "
                              "tube's fp64 mean and row_len its count after taking the row; -1, 0, 0 for a row that is not counted: a tube's score and length are those "
                              "of its last row. The walk is tuber_tube_link's kernel body. K > tuber_frame_match_max_dets(), K * (max_gap + 1) > "
                              "tuber_tube_link_max_active(), (slot_base + S) * K beyond an int32, bad sizes or pointers: negative, nothing launched, the state untouched.",
    "tuber_tube_link_state_bytes": "bytes of the state buffer of tuber_tube_link_stream for C classes (40 per (class, lane): C * 64 * 40); 0 for C <= 0.",
    "tuber_tube_link_max_active":"simultaneously active tubes of one (video, class) tuber_tube_link takes: max rows per slot x (max_gap + 1) (64).",
    "tuber_tube_match": "video-mAP on the device, matching step (evaluation.VideoMAP.match): the tuber_tube_link outputs against ground-truth tubes given as gt_box [G][4] fp64 / "
                        "gt_cls [G] / gt_tube [G] (the rank of the row's tube among the tube ids of its (video, class), ascending; one row per (slot, class, tube)) in slot order "
                        "with gt_off DEVICE int[S + 1]. stIoU(d, g) = sum over the shared slots of the fp64 IoU / |slots of d or g|, 0 without a shared slot. Per (video, class) the "
                        "tubes of at least min_len detections are visited by descending score (equal scores by ascending head); per threshold (thresholds DEVICE double[T]) a tube "
                        "takes the not yet taken ground-truth tube of largest stIoU (the first maximum) and is a true positive iff that stIoU >= threshold. tube_flag [T][N] bytes: "
                        "1 true positive, 0 false positive, 2 not counted (not a head, shorter than min_len), 3 a (video, class) beyond the bounds. work: caller-owned "
                        "double[N * max(max_gt_tubes, 1)]. max_rows / max_gt_rows / max_gt_tubes: largest rows and ground-truth rows per slot, ground-truth tubes per (video, "
                        "class). T > tuber_tube_match_max_thresholds(), max_gt_tubes > tuber_tube_match_max_gt(), max_rows > tuber_frame_match_max_dets(), max_gt_rows > "
                        "tuber_frame_match_max_gt(), bad sizes or pointers: negative, nothing launched. One wave per (video, class), sums in slot order: the same bits every run.",
    "tuber_tube_nms": "spatio-temporal tube NMS on the device (evaluation.tube_nms: the definition; the 3-D NMS the ACT-detector protocol runs over the tubes of a "
                      "(video, class) before video-mAP): the tuber_tube_link / tuber_tube_link_ranked outputs as tuber_tube_match reads them -- the validation store in "
                      "layout order, or a padded [S][K] store with slot_off = arange(S + 1) * K and V = 1. stIoU(d, e) = sum over the slots both tubes have a row in, "
                      "ascending, of the fp64 IoU of the two fp32 boxes / |slots of d or e|, 0 without a shared slot. Per (video, class) the tubes of at least min_len "
                      "detections are visited by descending score (NaN last, equal scores by ascending head); a tube is suppressed iff its stIoU with a tube KEPT "
                      "before it is > nms_iou (strictly), so a suppressed tube suppresses nothing. tube_keep [N] bytes: 1 kept head, 0 suppressed head, 2 not a head "
                      "or shorter than min_len, 3 at the heads of a (video, class) in which more than tuber_tube_link_max_active() tubes are live (head <= slot <= "
                      "tube_last) at one slot: nothing decided there. A row whose row_head lies outside [first row of its video, the row] or is no head row of the "
                      "row's class is not counted. work: caller-owned, tuber_tube_nms_work_bytes(N) bytes, 16-byte aligned. One wave per (video, class): the live "
                      "tubes in lanes, the pair sums in a [64][64] LDS table accumulated in slot order, a pair recorded when the first of its tubes ends, then the "
                      "greedy pass; no atomics on floating-point data, plain vector stores, the same bits every run. max_rows > tuber_frame_match_max_dets(), "
                      "min_len < 1, nms_iou NaN or outside [0, 1], N > S * max_rows, negative sizes, a null pointer or a misaligned work: negative, nothing launched, "
                      "nothing written. N == 0 or V == 0: 0, nothing written.",
    "tuber_tube_nms_work_bytes": "bytes of the scratch of tuber_tube_nms for N rows: 64 partner heads and one status word (int32) per row, rounded up to 16; 0 for N <= 0.",
    "tuber_tube_dense": "dense action tubes on the device (evaluation.dense_rows: the definition; the per-frame tubes of the UCF101-24 / JHMDB protocol, which the "
                        "ACT-detector tooling also fills by interpolating between key detections): a box and a score on every frame between two linked key "
                        "detections of ONE video's padded [S][K] store. det_box [S * K][4] / det_score [S * K] fp32, row_head [S * K] as tuber_tube_link_ranked "
                        "wrote it, slot_frame [S] the frame number of every key ordinal, strictly ascending; G >= the most frames a row can own, max(1, max over s "
                        "of slot_frame[min(s + max_gap + 1, S - 1)] - slot_frame[s]), a host integer. Out per row r of slot s: row_next, the first row with r's "
                        "head in the slots s + 1 .. s + max_gap + 1 (-1: none); row_span g = slot_frame[its slot] - slot_frame[s] (1 without a successor; 0, with "
                        "row_next -1, for a row with head < 0); dense_box [S * K][G][4] / dense_score [S * K][G] fp32 at j < g, frame slot_frame[s] + j: the row's "
                        "own bytes at j = 0, float(double(a) + (double(b) - double(a)) * (double(j) / double(g))) per coordinate and for the score behind it (a "
                        "the row, b its successor; every operation rounded on its own, a NaN result 0x7FC00000): the definition's bits. Nothing is written at j "
                        ">= g. g < 1 or g > G (unsorted slot_frame, a G too small): row_span -1 and nothing else, the caller answers with the definition. One "
                        "wave per row: the candidate heads in lanes and one ballot, then lanes j, j + 64, ... write a 16-byte box and a score each; no LDS, no "
                        "atomics, plain vector stores. K > tuber_frame_match_max_dets(), K * (max_gap + 1) > tuber_tube_link_max_active(), S * K * G beyond an "
                        "int32, G < 1, K < 1, negative sizes, a null pointer, det_box / dense_box not 16-byte or another pointer not 4-byte aligned: "
                        "TUBER_EINVAL, nothing launched, nothing written. S == 0: 0, no launch.",
    "tuber_tube_crops": "crops of action tubes and actor tracks out of the resident video (crops.crop_rows: the definition; what RoIAlign with a sampling_ratio does "
                        "to an image, and torch's grid_sample(mode=bilinear, padding_mode=border, align_corners=False) to within fp64 rounding): row r of a crop "
                        "table -- frame_index int32 [R], boxes fp32 [R][4] xyxy in source-video pixels, pixel j covering [j, j + 1) -- resampled to h x w out of "
                        "frames uint8 [N][H][W][3] (packed, at any byte alignment). fx = W / W0, fy = H / H0: the host's fp64 quotients of the frame size by the "
                        "size the boxes refer to; scale > 0 enlarges a box about its centre; samples = s: an output pixel is the mean of an s x s regular grid of "
                        "bilinear samples. Per axis, in fp64, every operation rounded on its own: cx = (x1 + x2) * 0.5; bw = (x2 - x1) * scale; X1 = (cx - bw * "
                        "0.5) * fx; sx = (bw * fx) / double(w * s); sample column c: u = X1 + (c + 0.5) * sx - 0.5 clamped to [0, W - 1] (edge replication; a "
                        "NaN, which only an overflowing scale gives, to 0), j0 = floor(u), j1 = min(j0 + 1, W - 1), a = u - j0; per channel top = p[i0][j0] + "
                        "(p[i0][j1] - p[i0][j0]) * a, bot likewise on line i1, val = top + (bot - top) * b; pixel (i, j): acc = 0, then acc = acc + val(i * s + "
                        "dy, j * s + dx) for dy, for dx; byte = floor(acc / double(s * s) + 0.5): the definition's bytes. lut == NULL: out is uint8 [R][h][w][3] "
                        "at any byte alignment. lut != NULL: the fp32 [3][256] mean/std table tuber_video_clips reads, and out is fp32 [R][3][h][w] with "
                        "out[r][ch][i][j] = lut[ch][byte] -- a crop pixel is what a clip pixel of the same byte would be. valid uint8 [R]: 0 at a row whose "
                        "frame_index lies outside [0, N) or whose box has a coordinate that is not finite; its bytes are 0. x2 < x1 mirrors, a box of no area gives "
                        "a constant. A workgroup per row and band of output lines (at most 2040 output bytes); the coordinates and weights of the sample columns "
                        "and lines once in LDS tables; per pass over the sample lines the span of the two source lines each one needs staged into LDS with "
                        "aligned dword loads; aligned dword stores over the flat output with a byte head and tail per band (16-byte stores in the table form); "
                        "no atomics, plain vector stores, nothing written outside the R rows and valid. W > tuber_tube_crops_limits(0), h or w > limits(1), "
                        "samples > limits(2); h, w, samples, H or W below 1; negative N or R; R * bands beyond an int32; fx, fy or scale not finite or not "
                        "positive; a null pointer; boxes not 16-byte, frame_index, lut or an fp32 out not 4-byte aligned: TUBER_EINVAL, nothing launched, "
                        "nothing written. R == 0: 0, no launch, the pointers are not inspected.",
    "tuber_tube_crops_limits": "bounds of tuber_tube_crops: which = 0 the largest frame width W (4096: two staged lines of 3 * W bytes and the column table fit a "
                               "workgroup's LDS), 1 the largest h or w of a crop (512), 2 the largest samples (4); anything else -1.",
    "tuber_tube_match_max_gt": "ground-truth tubes per (video, class) tuber_tube_match takes (32).",
    "tuber_tube_match_max_thresholds": "thresholds per call tuber_tube_match takes (16).",
    "tuber_detect_ava": "ranked detections of an AVA eval forward in ONE launch (PostProcessAVA, models/criterion.py:447-482, the post-processor models/tuber_ava.py builds; "
                        "box_cxcywh_to_xyxy utils/box_ops.py:9-13; then threshold and top-K): pb = softmax(pred_logits_b)[1]; a query passes when pb > actor_thr; "
                        "score(q, c) = sigmoid(logit) * pb; candidates: (q, c) of a passed query with a score that is not NaN and >= score_thr; the best K by score "
                        "descending, then q, then c ascending. pred_logits [B][Qtot][C], pred_logits_b [B][lb_rows][NB] (lb_rows = Qtot or 1), pred_boxes [B][Qtot][4], each "
                        "fp32 or bf16 by its bit of dtypes (1, 2, 4), converted on load; sizes [B][2] fp32 (h, w); q_begin DEVICE int[B] or NULL: where the clip's Qs "
                        "queries start. Out: det_box [B][K][4] xyxy pixels (bit-identical to decode()'s), det_score, det_aux (pb) [B][K] fp32, det_label, det_query [B][K] "
                        "int, det_count [B] = min(det_total, K), det_total [B]; rows from det_count on: box 0, score 0, aux 0, label -1, query -1. One workgroup per clip, "
                        "the clip's order keys sorted in LDS: no atomics, no workspace, no host synchronisation. Beyond tuber_detect_limits: -2, nothing launched.",
    "tuber_detect_top1": "ranked detections of a JHMDB / UCF101-24 eval forward in ONE launch (PostProcess, models/tuber_jhmdb.py:357-389, plus the counted-once rule of "
                         "evaluates/evaluate_ucf.py:109-126): a query's label is the first maximum of its fp32 logit row over the C + 1 columns (a NaN counting as a maximum), "
                         "its score that column's softmax probability; not a candidate when the label is the no-object column C, the score is NaN or < score_thr; the best K "
                         "by score descending, then q ascending; det_aux: the visibility probability softmax(pred_logits_b)[1]. Arguments and outputs as tuber_detect_ava.",
    "tuber_detect_limits": "bounds of tuber_detect_ava / tuber_detect_top1: which = 0 the largest Qs * C (4096), 1 the largest K (1024), 2 the largest NB (8).",
    "tuber_detect_actors": "actor decode of an AVA eval forward in ONE launch (detect.decode_actors_host: the definition; the reference has no such path, its "
                           "PostProcessAVA, models/criterion.py:447-482, returns the dense table): an ACTOR is a query of the clip's slice whose pb = "
                           "softmax(pred_logits_b)[1] is not NaN and > actor_thr; the best A by pb descending, then query ascending, are kept, each with its box and "
                           "its WHOLE action row. Inputs as tuber_detect_ava. Out: det_box [B][A][4] xyxy pixels (bit-identical to decode()'s), det_actor [B][A] fp32 "
                           "(pb), det_query [B][A] int, det_actions [B][A][C] fp32 = sigmoid(logit) * pb for EVERY class, unthresholded, bit-identical to "
                           "tuber_detect_ava's score of the same (query, class), a NaN logit staying NaN; det_count [B] = min(det_total, A), det_total [B]; rows from "
                           "det_count on: box 0, actor 0, query -1, actions 0. One workgroup per clip, the order keys fmap_key(pb, q) sorted in LDS, the action rows "
                           "written by the whole workgroup with 16-byte stores where C % 4 == 0: no atomics. Beyond tuber_detect_actors_limits (or A * C beyond an "
                           "int32): -2, nothing launched; bad sizes or pointers, a NaN threshold: -1.",
    "tuber_detect_actors_limits": "bounds of tuber_detect_actors: which = 0 the largest Qs (1024), 1 the largest A (1024), 2 the largest NB (8).",
    "tuber_track_actions": "per-track and temporally smoothed action scores of ONE video's linked actor rows (evaluation.actor_tracks: the definition): actions "
                           "[S * A][C] fp32 with row r = slot * A + a; row_head / tube_last [S * A] as tuber_tube_link_ranked wrote them with class_num = 1. Out: "
                           "row_smooth [S * A][C] fp64: the mean over the rows of the row's track at most `window` slots away; at head rows track_mean [S * A][C] "
                           "fp64 and track_peak [S * A][C] fp32 (the maximum, a NaN staying); zeros at rows with head -1 and, for the track outputs, at rows that are "
                           "no head. Every sum is fp64, sequential in slot order, then one division: the definition's bits. A workgroup per row, a wave per 64 "
                           "classes, a row's track member in a slot found by one ballot over the slot's A heads; no atomics. A or C beyond "
                           "tuber_track_actions_limits, S * A beyond an int32, bad sizes or pointers: negative, nothing launched.",
    "tuber_track_actions_limits": "bounds of tuber_track_actions: which = 0 the largest A (64, the linker's), 1 the largest C (4096).",
    "tuber_track_actions_stream": "tuber_track_actions for ONE video whose key frames arrive in pieces (evaluation.ActorTracker: the definition; "
                                  "video.VideoStream(actors=A)). This call takes the S new slots slot_base .. slot_base + S - 1 of A rows each: actions [S * A][C] fp32, "
                                  "row_head [S * A] as tuber_tube_link_stream wrote it for the same slots with C = 1, K = A and the same slot_base. Out: row_mean "
                                  "[S * A][C] fp64 / row_peak [S * A][C] fp32, the track's running mean (fp64 sum in slot order / count) and maximum (a NaN staying) "
                                  "after taking the row: at a track's last row tuber_track_actions' track_mean / track_peak, bit for bit; smooth [(hi - lo) * A][C] "
                                  "fp64: tuber_track_actions' row_smooth of the slots lo = max(slot_base - window, 0) .. hi = flush ? slot_base + S : "
                                  "max(slot_base + S - window, lo) (evaluation.smooth_range) -- a smoothed row looks window slots ahead, so it is emitted window slots "
                                  "late; flush != 0 marks the end of the video. Zeros at rows with head -1. state: caller-owned, "
                                  "tuber_track_stream_state_bytes(A, C, max_gap, window) bytes, 16-byte aligned, all zero = a new video: a ring of the last H = max(2 * "
                                  "window, max_gap + 1) + 1 slots, entry ordinal % H, per row the head and the count, per (row, class) the running fp64 sum, the fp32 "
                                  "peak and the fp32 action. Every pushed slot, an empty one included, writes its entry and the kernel knows slot_base, so an entry "
                                  "of an ordinal below 0 or of a slot not yet pushed is never consulted. One wave per 64 classes, each with its OWN copy of the head "
                                  "/ count records in front of its class columns: no workgroup reads what another one writes, no atomics, plain vector stores. A, C "
                                  "or window beyond tuber_track_stream_limits, A * (max_gap + 1) > tuber_tube_link_max_active(), (slot_base + S) * A beyond an int32, "
                                  "bad sizes, a null or misaligned pointer, negative arguments: TUBER_EINVAL, nothing launched, the state untouched, nothing written. "
                                  "S == 0 without flush: 0, no launch; with flush: the last min(window, slot_base) slots.",
    "tuber_track_stream_state_bytes": "bytes of the state buffer of tuber_track_actions_stream: per 64 classes, H * A head and count records (rounded up to 16 "
                                      "bytes) and H * A * 64 columns of 16 bytes, H = max(2 * window, max_gap + 1) + 1; 0 for arguments outside the bounds.",
    "tuber_track_stream_limits": "bounds of tuber_track_actions_stream: which = 0 the largest A (64, the linker's), 1 the largest C (4096), 2 the largest window "
                                 "(31: a ring of 63 slots); anything else -1.",
    "tuber_tensor_stats_chunk":"largest number of elements in one chunk of tuber_tensor_stats (a multiple of 64).",
    "tuber_tensor_stats_tensor_bytes": "sizeof(TensorStatsTensor) as compiled (host-side layout check).",
    "tuber_tensor_stats_chunk_bytes": "sizeof(TensorStatsChunk) as compiled (host-side layout check).",
    "tuber_grad_accum": "gradient accumulation over m micro-batches (DistributedDataParallel's mean over ranks reproduced on fewer GPUs: the mean of "
                        "independent per-rank backward passes, utils/model_utils.py:47-49) over a DEVICE table of nwin [begin, end) int64 windows of the flat "
                        "fp32 gradient buffer, in ONE launch: mode 0 acc = g, mode 1 acc += g, mode 2 g = (acc + g) * scale (scale_dev[0] when given). "
                        "Fixed order: sequential fp32 sum, then one multiply. g and acc 16-byte aligned.",
    "tuber_bn_stats_copy": "snapshot (restore = 0: arena <- buffers) or restore (restore = 1: buffers <- arena) of BatchNorm running statistics "
                           "(running_mean, running_var, num_batches_tracked of nn.BatchNorm3d, models/backbones/ir_CSN_152.py:46,56,64,154) in ONE launch over a "
                           "DEVICE table of nrows {address, arena offset in 32-bit words, words} int64 rows; max_words = the largest row.",
    "tuber_scale_f32": "x *= coef: gradient averaging after the RCCL all-reduce (DistributedDataParallel's mean, utils/model_utils.py:47-49).",
    "tuber_criterion_cost": "Hungarian matching cost C = w_bbox*L1 - w_giou*GIoU - w_class*p of every decoder layer at once, [L,B,Q,Tmax] fp32 "
                            "(HungarianMatcher.forward, models/detr/matcher.py:61-76 / matcher_ucf.py:61-78; generalized_box_iou utils/box_ops.py:41-65).",
    "tuber_criterion_loss": "all loss terms of all layers and their gradients w.r.t. logits / actor logits / boxes in one launch: AVA 3-way weighted CE + "
                            "weighted BCE (models/criterion.py:42-81), JHMDB (C+1)-way CE (:237-262), L1 + GIoU box losses (:97-117).",
    "tuber_cast_f32_bf16": "fp32 -> bf16 copy (bf16 shadow of the fp32 master weights).",
    "tuber_cast_transpose": "W[R][C] fp32 -> W^T[C][ldt] bf16 (B operand of the data-gradient GEMM).",
    "tuber_rows_gather_sum": "out[(a,b,c)] = mul * sum_d in[a*sa+b*sb+c*sc+d*sd] over rows of E bf16: temporal AvgPool3d((4,1,1)) "
                             "(backbone_builder.py:44,73), its backward (broadcast), the x6 replication of src_c (tuber_ava.py:133) and its backward (sum).",
    "tuber_axpby": "out = alpha*a + beta*b (bf16): with_pos_embed adds (transformer.py:150-151), gradient accumulation.",
    "tuber_dropout": "y = keep ? x/(1-p) : 0 with a stateless hash RNG keyed by (seed, index); applying it to a gradient with the same seed is the backward.",
    "tuber_sigmoid_fwd": "boxes = sigmoid(bbox_embed(hs)) (tuber_ava.py:142).",
    "tuber_sigmoid_bwd": "dx = dy*y*(1-y).",
    "tuber_relu_mask": "dx = dy*[h>0] (ReLU backward from the saved activation; FFN and MLP hidden layers).",
    "tuber_multi_transpose_bf16": "every GEMM weight W[R][C] -> W^T[C][ldt] (bf16 shadow of the parameters -> bf16: the B operand of the data-gradient GEMMs, autograd of "
                                  "nn.Conv3d(k=1) / nn.Linear) in one launch over a device table {src_off,dst_off,R,C,ldt,tile_begin,tiles_x,pad} of 64 x 64 tiles.",
    "tuber_cast_pad_rows": "src[R][C] fp32 -> dst[R][ldd] bf16 with zero-filled pad columns (stem 441->448 taps, head gradients).",
    "tuber_rows_scatter_add": "dst[map(m)] += src[m] over the strided (n,t*st,h*ss,w*ss) row map: input gradient of a strided down_sample conv (ir_CSN_152.py:155-161).",
    "tuber_posenc": "PositionEmbeddingSine_3D (models/transformer/position_encoding.py:32-72) of a (B,T,H,W) padding mask, token-major bf16.",
}

HEADER = '''/* tuber_hip.h -- C ABI of libtuber_hip.so: the MI355X (gfx950) kernels behind the TubeR forward/backward path.
 *
 * GENERATED by tubelet_transformer_amd/csrc/gen_header.py from the extern "C" definitions in csrc/*.hip.
 *
 * The reference (amazon-science/tubelet-transformer) has no FFI or operator-plugin boundary: its hot path is stock
 * torch.nn calls (SURVEY.md section 8b).  This ABI is therefore build-defined: one launcher per kernel family, each
 * citing the reference call site(s) whose arithmetic it replaces.  Conventions:
 *   - plain pointers to DEVICE memory + explicit sizes / leading dimensions (in elements); no torch types;
 *   - activations are row-major [rows, channels] bf16 (NDHWC / token-major), master weights and statistics fp32;
 *   - the callee never allocates: outputs, saved tensors and workspaces (`partial`, `st0`, ...) are caller-owned,
 *     sized with the *_rows / *_slabs / *_blocks helper calls;
 *   - every launcher enqueues on `stream` and returns 0, a negative argument-check code (TUBER_EINVAL = -1) or the
 *     positive hipError_t of a failed launch; nothing throws across the ABI.
 */
#ifndef TUBER_HIP_H
#define TUBER_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* one clip of tuber_clip_prepare (device memory, 56 bytes) */
typedef struct TuberClipDesc {
    long long src_off;   /* byte offset of the clip's first frame in `frames` (uint8 [T][H][W][3]) */
    int H, W;            /* frame size */
    int y1, x1, h, w;    /* crop window in the (flipped) frame: output (y,x) reads (y1+y, x1+x) */
    int flip, jitter;    /* horizontal flip before the crop; HSV colour jitter on/off */
    int hue, sat, val;   /* ColorJitter shifts (hue in OpenCV half-degrees) */
    int pad_;
} TuberClipDesc;

'''
FOOTER = '''
#ifdef __cplusplus
}
#endif
#endif /* TUBER_HIP_H */
'''


def prototypes():
    out = []
    for f in sorted(glob.glob(os.path.join(HERE, "*.hip")) + glob.glob(os.path.join(HERE, "*.cpp"))):
        s = open(f).read()
        for m in re.finditer(r'^(int|long|const char\*) (tuber_\w+)\(([^)]*)\)\s*\{', s, re.M):
            out.append((os.path.basename(f), m.group(1), m.group(2), " ".join(m.group(3).split())))
    return out


def wrap(text, width=116, indent=" * "):
    words, lines, cur = text.split(), [], ""
    for w in words:
        if len(cur) + len(w) + 1 > width:
            lines.append(cur)
            cur = w
        else:
            cur = (cur + " " + w).strip()
    lines.append(cur)
    return "\n".join(indent + l for l in lines)


def main():
    parts = [HEADER]
    last = None
    for f, ret, name, args in prototypes():
        if f != last:
            parts.append("/* ---- %s ---- */\n" % f)
            last = f
        parts.append("/*\n%s\n */\n" % wrap(DOC.get(name, "(undocumented)")))
        parts.append("%s %s(%s);\n\n" % (ret, name, args if args else "void"))
    parts.append(FOOTER)
    os.makedirs(os.path.join(ROOT, "include"), exist_ok=True)
    open(os.path.join(ROOT, "include", "tuber_hip.h"), "w").write("".join(parts))
    missing = [n for _, _, n, _ in prototypes() if n not in DOC]
    if missing:
        print("undocumented:", missing)


if __name__ == "__main__":
    main()
