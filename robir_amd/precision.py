"""One switch for the arithmetic of every MLP kernel.

  ROBIR_PRECISION=exact  (default)  not narrower than the reference's fp32: the fused light-visibility kernel carries every
                                    fp32 operand exactly as three f16 pieces (six MFMA products per multiply-add, three fp32
                                    accumulators: csrc/vis_diffuse_x6.hip; since round 6 the two outer products of the 2^-22 class from bf8
                                    copies of their operands, error against float64 unchanged: csrc/vis_diffuse_x6t.hip), and so do the SDF network (values and reverse-mode
                                    gradient), the colour network, the stand-alone visibility MLP, the 512-wide nets and the CESR
                                    nets (MLP mode "f16x6": csrc/sdf_x6.hip, sdf_back_x6.hip, color_x6.hip, vis_x6.hip, wide_x6.hip,
                                    cesr_x6.hip); the small auto-encoder decoders run on the f32-input MFMA.  ROBIR_MLP_PRECISION=fp32 puts every stand-alone MLP on the f32-input MFMA;
  ROBIR_PRECISION=split             22-bit operands: (hi, lo) f16 pairs, three products per multiply-add, fp32 accumulate --
                                    2x the throughput, parity-tested against the oracle at the same 1e-4 (tests/test_precision_gpu.py),
                                    guarded by the activation-range sentinel (ops.range_check).
  ROBIR_PRECISION=f16               the labelled THROUGHPUT policy `BASELINE.json configs[4]` names ("fp16 MLP weights on MFMA"):
                                    the light-visibility MLP in PLAIN f16 -- one f16 MFMA product per multiply-add, f16 weights
                                    (round-to-nearest) and f16 activations (truncated between the layers), fp32 accumulation
                                    (csrc/vis_diffuse_f16p.hip, vis_diffuse_f16t.hip) -- the two CESR nets likewise since round 6
                                    (csrc/cesr_f16.hip: 52 % of config 5) -- and, since round 5, every other net in SPLIT
                                    precision (f16 hi/lo weight and activation pairs, three products: the parity-tested family of
                                    `split`, legacy library) instead of the exact-operand kernels: no one-product kernels exist for
                                    those nets, and a throughput policy that left them at six products gave the CESR stage 18 %.
                                    NARROWER than the reference's fp32: never a default, never a parity claim; its measured
                                    error against a float64 evaluation is in DESIGN.md and printed by tests/test_precision_gpu.py.
  ROBIR_PRECISION=f16-vis           round 4's meaning of `f16`, kept selectable: plain f16 for the light-visibility MLP only,
                                    every other net on the exact-operand kernels -- needs the default library only.
ROBIR_VIS_PRECISION / ROBIR_MLP_PRECISION override the two halves of the policy separately (A/B runs, tests).

Operand range of `exact` (tests/split_model.py holds the constants, tests/test_split_cpu.py establishes them on a numpy restatement of the
splits, tests/test_mlp_gpu.py and tests/test_precision_gpu.py hold the device to them; DESIGN section 6 has the measurements):
  six f16 products (every stand-alone f16x6 kernel; f16x6-1t)   a weight or activation v is carried EXACTLY as h + m 2^-11 + l 2^-22 for
                                    2^-23 <= |v| <= 65504 (EXACT_MIN, F16_MAX) and for +-0 -- f16 subnormals included, and through the binade
                                    [32768, 65504) where the m piece of an activation relies on the round-toward-zero clamp at 65504.
                                    Below 2^-23 the absolute error is at most min(|v|, 2^-47) (BELOW_WINDOW_ABS_ERR = 7.1e-15).  From
                                    65504 on the leading piece saturates and ops.range_check reports the kernel (packing refuses such weights).
  bf8 form (the shipped light-visibility kernel, f16x6-pt / f16x6-stream: h.xl and l.xh from e5m2 copies)   the copy of the third piece is
                                    bit-exact for 2^-15 <= |v| <= 65504 (BF8_L_EXACT_MIN; the first magnitude that fails is one fp32 unit
                                    below 2^-15, BF8_L_FIRST_FAIL): there l has at most three significant bits.  Below 2^-15 the operand
                                    is off by less than 2^-38 in absolute terms (BF8_BELOW_WINDOW_ABS_ERR = 3.6e-12): still fp32-like
                                    for typical activations down to ~2^-17, past the 1e-4 bar once they fall to ~2^-25.
"""
import os

POLICIES = {"exact": ("f16x6", "f16x6"), "split": ("f16x3-auto", "f16x3"), "f16": ("f16x1", "f16x3"), "f16-vis": ("f16x1", "f16x6")}
VIS_MODES = ("fp32", "f16x6", "f16x3-auto", "f16x3-v3", "f16x3-v2", "f16x3", "f16x1", "f16x6-1t", "f16x6-pt", "f16x6-stream")


VALID = {"ROBIR_MLP_PRECISION": (("f16x3", "fp32", "f16x6"), "f16x6, fp32 or f16x3"),
         "ROBIR_CESR_PRECISION": (("f16x1", "f16x3", "fp32", "f16x6"), "f16x1, f16x6, fp32 or f16x3"),
         "ROBIR_VIS_PRECISION": (VIS_MODES, "one of " + ", ".join(VIS_MODES))}


def check(variable, p):
    """p if it is a value of `variable`, else the ValueError (robir_amd.dispatch raises the same for a string handed to it directly)."""
    if p not in VALID[variable][0]:
        raise ValueError(f"{variable} must be {VALID[variable][1]}")
    return p


def policy():
    p = os.environ.get("ROBIR_PRECISION", "exact")
    if p not in POLICIES:
        raise ValueError("ROBIR_PRECISION must be exact, split, f16 or f16-vis")
    return p


def mlp_precision():
    """Arithmetic of the stand-alone MLP kernels (SDF, colour, visibility, 512-wide nets): 'f16x6' (exact three-piece operands where
    such a kernel exists -- SDF, colour, visibility MLP -- and the f32-input MFMA elsewhere), 'fp32' (f32-input MFMA everywhere) or
    'f16x3' (split precision)."""
    return check("ROBIR_MLP_PRECISION", os.environ.get("ROBIR_MLP_PRECISION") or POLICIES[policy()][1])


def cesr_precision():
    """Arithmetic of the two CESR nets (shadow_net, normal_net: training/train_cesr.py:106-110): 'f16x1' -- plain f16, ONE MFMA product per
    multiply-add (csrc/cesr_f16.hip, round 6; NARROWER than fp32) -- under ROBIR_PRECISION=f16, the policy `BASELINE.json configs[4]` names
    ("CESR stage full pipeline, fp16 MLP weights on MFMA"); else whatever mlp_precision() says.  ROBIR_CESR_PRECISION overrides (A/B runs)."""
    p = os.environ.get("ROBIR_CESR_PRECISION")
    if p is None:
        p = "f16x1" if (policy() == "f16" and not os.environ.get("ROBIR_MLP_PRECISION")) else mlp_precision()
    return check("ROBIR_CESR_PRECISION", p)


def vis_precision():
    """Arithmetic of the fused light-visibility kernel at import time of robir_amd.sg_render (its VIS_PRECISION attribute is
    what is read per call)."""
    return check("ROBIR_VIS_PRECISION", os.environ.get("ROBIR_VIS_PRECISION") or POLICIES[policy()][0])
