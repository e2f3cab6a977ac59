"""ctypes loader for librobir_hip.so (the C-ABI of include/robir_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails, we raise.
torch is imported first so that the process uses ONE HIP runtime (torch bundles libamdhip64.so.7; our library
resolves the same soname against the already-loaded copy).
"""
import ctypes
import os
import subprocess

import torch  # noqa: F401  (must precede the CDLL: pins the HIP runtime instance)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librobir_hip.so")
_lib = None

c_fp = ctypes.c_void_p
c_long = ctypes.c_long
c_int = ctypes.c_int
c_float = ctypes.c_float


class RobirHipError(RuntimeError):
    pass


LEGACY_PATH = os.path.join(_HERE, "librobir_hip_legacy.so")
_legacy = None
ABI_VERSION = 8
TRAIN_PATH = os.path.join(_HERE, "librobir_hip_train.so")
_train = None
TRAIN_ABI_VERSION = 1
VISTRAIN_PATH = os.path.join(_HERE, "librobir_hip_vistrain.so")
_vistrain = None
VISTRAIN_ABI_VERSION = 1
ILLUMTRAIN_PATH = os.path.join(_HERE, "librobir_hip_illumtrain.so")
_illumtrain = None
ILLUMTRAIN_ABI_VERSION = 1
CESRTRAIN_PATH = os.path.join(_HERE, "librobir_hip_cesrtrain.so")
_cesrtrain = None
CESRTRAIN_ABI_VERSION = 1
LIGHTFIT_PATH = os.path.join(_HERE, "librobir_hip_lightfit.so")
_lightfit = None
LIGHTFIT_ABI_VERSION = 1
TEXBAKE_PATH = os.path.join(_HERE, "librobir_hip_texbake.so")
_texbake = None
TEXBAKE_ABI_VERSION = 1
OBSERVE_PATH = os.path.join(_HERE, "librobir_hip_observe.so")
_observe = None
OBSERVE_ABI_VERSION = 1
PHOTOLOSS_PATH = os.path.join(_HERE, "librobir_hip_photoloss.so")
_photoloss = None
PHOTOLOSS_ABI_VERSION = 1
METRICS_PATH = os.path.join(_HERE, "librobir_hip_metrics.so")
_metrics = None
METRICS_ABI_VERSION = 1
RASTER_PATH = os.path.join(_HERE, "librobir_hip_raster.so")
_raster = None
RASTER_ABI_VERSION = 1
TEXFIT_PATH = os.path.join(_HERE, "librobir_hip_texfit.so")
_texfit = None
TEXFIT_ABI_VERSION = 1


def build(verbose=False, legacy=True):
    """Compile every HIP translation unit for gfx950 and link, in-tree, librobir_hip.so (the default library), librobir_hip_train.so (the
    training-side kernels, csrc/train/), librobir_hip_vistrain.so (the visibility network's backward, csrc/vistrain/),
    librobir_hip_illumtrain.so (the indirect-illumination lobe net's backward and the fused SG query, csrc/illumtrain/),
    librobir_hip_cesrtrain.so (the backward of the CESR stage's shadow_net / normal_net, csrc/cesrtrain/), librobir_hip_lightfit.so (the fit of
    the light SGs to an environment map, csrc/lightfit/), librobir_hip_texbake.so (baking into texture space, csrc/texbake/),
    librobir_hip_observe.so (multi-view observations of surface points, csrc/observe/), librobir_hip_photoloss.so (the tone curves' backward
    and the fused image loss, csrc/photoloss/), librobir_hip_metrics.so (PSNR / SSIM / normal error / albedo ratio, csrc/metrics/),
    librobir_hip_raster.so (the camera-space rasteriser and the G-buffer, csrc/raster/), librobir_hip_texfit.so (the fit of a baked atlas
    to views, csrc/texfit/) and -- legacy=True -- librobir_hip_legacy.so (the superset with the retired kernel
    generations, csrc/Makefile)."""
    # MAX_JOBS where the environment sets the build's share of the CPUs (os.cpu_count() is the whole machine's); never above 16
    jobs = str(max(1, min(16, int(os.environ.get("MAX_JOBS") or min(8, os.cpu_count() or 1)))))
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j", jobs, "all" if legacy else "default"],
                       capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RobirHipError("building librobir_hip.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


def _load(path, what):
    if not os.path.exists(path):
        raise RobirHipError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` " + what)
    L = ctypes.CDLL(path)
    L.rb_last_error.restype = ctypes.c_char_p
    for name in ("rb_packed_layer_floats", "rb_packed_layer_x6_floats", "rb_sdf_value_grad_scratch_floats",
                 "rb_sdf_value_grad_f32_scratch_floats", "rb_sg_shade_bwd_scratch_floats", "rb_mesh_groups"):
        if hasattr(L, name):
            getattr(L, name).restype = ctypes.c_long
    if L.rb_abi_version() != ABI_VERSION:
        raise RobirHipError(f"{os.path.basename(path)} ABI version mismatch")
    return L


def lib():
    """The default library (include/robir_hip.h): everything the `exact` / `f16` policies and the fp32 override run."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, "(robir_amd has no CPU fallback)")
    return _lib


def legacy():
    """The legacy library (include/robir_hip_legacy.h; `make -C robir_amd/csrc legacy`): loaded the first time a retired entry point is
    called -- ROBIR_PRECISION=split, ROBIR_SDF_FUSED_PE=0, the tests that compare kernel generations.  Its own copy of the process-wide
    state (range sentinel block, device caches)."""
    global _legacy
    if _legacy is None:
        _legacy = _load(LEGACY_PATH, "(the split-precision family and the other retired kernel generations live in the LEGACY library: build it "
                                     "with `make -C robir_amd/csrc legacy` or ROBIR_BUILD_LEGACY=1.  ROBIR_PRECISION=split needs it, and so does "
                                     "ROBIR_PRECISION=f16 for every net but the light-visibility MLP -- ROBIR_PRECISION=f16-vis and the default "
                                     "policy ROBIR_PRECISION=exact do not; current policy: " + os.environ.get("ROBIR_PRECISION", "exact") + ")")
        if os.environ.get("ROBIR_SDF_RING_WAVES") in ("4", "8"):      # value rows of the split SDF net: csrc/sdf_ring8.hip | sdf_ring.hip
            _legacy.rb_sdf_ring_waves(int(os.environ["ROBIR_SDF_RING_WAVES"]))
    return _legacy


def _load_aux(path, abi, prefix, long_queries, target, title, serves):
    """An auxiliary library: its own file, symbol prefix, ABI version, last-error function, `long`-returning queries and not-found message
    -- a missing file is reported as such, never as a missing legacy entry point -- and never resolved against another library."""
    if not os.path.exists(path):
        raise RobirHipError(f"{path} not found: the {title} ({serves}) is built by `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"or `make -C robir_amd/csrc {target}` -- there is no PyTorch fallback for its kernels")
    L = ctypes.CDLL(path)
    L.prefix = prefix
    getattr(L, prefix + "last_error").restype = ctypes.c_char_p
    for name in long_queries:
        getattr(L, name).restype = ctypes.c_long
    if getattr(L, prefix + "abi_version")() != abi:
        raise RobirHipError(f"librobir_hip_{target}.so ABI version mismatch")
    return L


def aux_error(L):
    """The last-error string of an auxiliary library (every library keeps its own)."""
    return getattr(L, L.prefix + "last_error")().decode()


def _call_aux(L, name, *args):
    fn = getattr(L, name, None)
    if fn is None:
        raise RobirHipError(f"{name} is not exported by {os.path.basename(L._name)}")
    rc = fn(*args)
    if rc != 0:
        raise RobirHipError(f"{name} failed ({rc}): {aux_error(L)}")


def train():
    """The training library (include/robir_hip_train.h; `make -C robir_amd/csrc train`): the reverse mode of the spec auto-encoder."""
    global _train
    if _train is None:
        _train = _load_aux(TRAIN_PATH, TRAIN_ABI_VERSION, "rb_train_", ("rb_train_ae_bwd_scratch_bytes",), "train", "TRAINING library",
                           "material-network gradients, robir_amd/ae_autograd.py")
    return _train


def call_train(name, *args):
    """An entry point of the training library."""
    _call_aux(train(), name, *args)


def vistrain():
    """The visibility-training library (include/robir_hip_vistrain.h; `make -C robir_amd/csrc vistrain`): the reverse mode of VisNetwork."""
    global _vistrain
    if _vistrain is None:
        _vistrain = _load_aux(VISTRAIN_PATH, VISTRAIN_ABI_VERSION, "rb_vt_", ("rb_vt_vis_bwd_scratch_bytes",), "vistrain",
                              "VISIBILITY-TRAINING library librobir_hip_vistrain.so", "visibility-network gradients, robir_amd/vis_autograd.py")
    return _vistrain


def call_vistrain(name, *args):
    """An entry point of the visibility-training library."""
    _call_aux(vistrain(), name, *args)


def illumtrain():
    """The illumination-training library (include/robir_hip_illumtrain.h; `make -C robir_amd/csrc illumtrain`): the reverse mode of
    IndirctIllumNetwork's lobe net, the fused SG query and its reverse."""
    global _illumtrain
    if _illumtrain is None:
        _illumtrain = _load_aux(ILLUMTRAIN_PATH, ILLUMTRAIN_ABI_VERSION, "rb_it_", ("rb_it_lobe_bwd_scratch_bytes",), "illumtrain",
                                "ILLUMINATION-TRAINING library librobir_hip_illumtrain.so",
                                "indirect-illumination gradients and the SG query, robir_amd/illum_autograd.py")
    return _illumtrain


def call_illumtrain(name, *args):
    """An entry point of the illumination-training library."""
    _call_aux(illumtrain(), name, *args)


def cesrtrain():
    """The CESR-training library (include/robir_hip_cesrtrain.h; `make -C robir_amd/csrc cesrtrain`): the reverse mode of the CESR stage's
    shadow_net and normal_net."""
    global _cesrtrain
    if _cesrtrain is None:
        _cesrtrain = _load_aux(CESRTRAIN_PATH, CESRTRAIN_ABI_VERSION, "rb_ct_", ("rb_ct_cesr_bwd_scratch_bytes",), "cesrtrain",
                               "CESR-TRAINING library librobir_hip_cesrtrain.so", "shadow_net / normal_net gradients, robir_amd/cesr_autograd.py")
    return _cesrtrain


def call_cesrtrain(name, *args):
    """An entry point of the CESR-training library."""
    _call_aux(cesrtrain(), name, *args)


def lightfit():
    """The light-fitting library (include/robir_hip_lightfit.h; `make -C robir_amd/csrc lightfit`): the reverse mode of the SG environment
    map, the fused steps of the fit and the area down-sample."""
    global _lightfit
    if _lightfit is None:
        _lightfit = _load_aux(LIGHTFIT_PATH, LIGHTFIT_ABI_VERSION, "rb_lf_", ("rb_lf_scratch_bytes", "rb_lf_groups"), "lightfit",
                              "LIGHT-FITTING library librobir_hip_lightfit.so", "light SGs of an environment map, robir_amd/lightfit.py")
    return _lightfit


def call_lightfit(name, *args):
    """An entry point of the light-fitting library."""
    _call_aux(lightfit(), name, *args)


def texbake():
    """The texture-baking library (include/robir_hip_texbake.h; `make -C robir_amd/csrc texbake`): the per-triangle UV atlas, the UV-space
    rasteriser, attribute interpolation, border dilation and the surface sampler."""
    global _texbake
    if _texbake is None:
        _texbake = _load_aux(TEXBAKE_PATH, TEXBAKE_ABI_VERSION, "rb_tb_", ("rb_tb_atlas_cell",), "texbake",
                             "TEXTURE-BAKING library librobir_hip_texbake.so", "material textures of an extracted mesh, robir_amd/texture.py")
    return _texbake


def call_texbake(name, *args):
    """An entry point of the texture-baking library."""
    _call_aux(texbake(), name, *args)


def observe():
    """The observation library (include/robir_hip_observe.h; `make -C robir_amd/csrc observe`): the inverse projection of surface points into
    the training views with its colour and mask fetch, the choice of n_obs views per point and the fused weighted colour statistics."""
    global _observe
    if _observe is None:
        _observe = _load_aux(OBSERVE_PATH, OBSERVE_ABI_VERSION, "rb_ob_", (), "observe",
                             "OBSERVATION library librobir_hip_observe.so", "multi-view observations of surface points, robir_amd/observe.py")
    return _observe


def call_observe(name, *args):
    """An entry point of the observation library."""
    _call_aux(observe(), name, *args)


def photoloss():
    """The photometric-loss library (include/robir_hip_photoloss.h; `make -C robir_amd/csrc photoloss`): the reverse mode of ACESToneMapping's
    curves and the fused masked image loss with its gradient."""
    global _photoloss
    if _photoloss is None:
        _photoloss = _load_aux(PHOTOLOSS_PATH, PHOTOLOSS_ABI_VERSION, "rb_pl_", ("rb_pl_groups", "rb_pl_scratch_bytes"), "photoloss",
                               "PHOTOMETRIC-LOSS library librobir_hip_photoloss.so",
                               "tone-map gradients and the image loss, robir_amd/tonemap_autograd.py")
    return _photoloss


def call_photoloss(name, *args):
    """An entry point of the photometric-loss library."""
    _call_aux(photoloss(), name, *args)


def metrics():
    """The metrics library (include/robir_hip_metrics.h; `make -C robir_amd/csrc metrics`): the fp64 sums behind MSE / MAE / PSNR / the albedo
    ratio, the angular error of two normal fields and SSIM, V views per launch."""
    global _metrics
    if _metrics is None:
        _metrics = _load_aux(METRICS_PATH, METRICS_ABI_VERSION, "rb_mt_",
                             ("rb_mt_groups", "rb_mt_ssim_tiles", "rb_mt_pair_scratch_bytes", "rb_mt_angular_scratch_bytes",
                              "rb_mt_ssim_scratch_bytes"), "metrics", "METRICS library librobir_hip_metrics.so",
                             "PSNR, SSIM, normal error and albedo ratio of rendered views, robir_amd/metrics.py")
    return _metrics


def call_metrics(name, *args):
    """An entry point of the metrics library."""
    _call_aux(metrics(), name, *args)


def raster():
    """The rasteriser library (include/robir_hip_raster.h; `make -C robir_amd/csrc raster`): the projection of a mesh's vertices, tile binning,
    the camera-space rasteriser with its depth test and the G-buffer with its plane fetch."""
    global _raster
    if _raster is None:
        _raster = _load_aux(RASTER_PATH, RASTER_ABI_VERSION, "rb_rs_", (), "raster", "RASTERISER library librobir_hip_raster.so",
                            "views of a baked mesh, robir_amd/meshrender.py")
    return _raster


def call_raster(name, *args):
    """An entry point of the rasteriser library."""
    _call_aux(raster(), name, *args)


def texfit():
    """The atlas-fitting library (include/robir_hip_texfit.h; `make -C robir_amd/csrc texfit`): the taps that linearise the mesh view's plane
    fetch, the fetch formed from them, its transpose as a gather and lazy Adam on the touched texels."""
    global _texfit
    if _texfit is None:
        _texfit = _load_aux(TEXFIT_PATH, TEXFIT_ABI_VERSION, "rb_tf_", (), "texfit", "ATLAS-FITTING library librobir_hip_texfit.so",
                            "fitting a baked atlas to views, robir_amd/texfit.py")
    return _texfit


def call_texfit(name, *args):
    """An entry point of the atlas-fitting library."""
    _call_aux(texfit(), name, *args)


def legacy_loaded():
    return _legacy is not None


def resolve(name):
    """(library, function) of an entry point: the default library if it exports `name`, else the legacy one."""
    L = lib()
    fn = getattr(L, name, None)
    if fn is None:
        L = legacy()
        fn = getattr(L, name, None)
        if fn is None:
            raise RobirHipError(f"{name} is exported by neither librobir_hip.so nor librobir_hip_legacy.so")
    return L, fn


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return ctypes.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "robir_amd kernels need contiguous device tensors"
    return ctypes.c_void_p(t.data_ptr())


def call_legacy(name, *args):
    """An entry point of the LEGACY library even where the default one exports the same name (rb_dvis_fused with precision 5)."""
    L = legacy()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise RobirHipError(f"{name} failed ({rc}): {L.rb_last_error().decode()}")


def call(name, *args):
    L, fn = resolve(name)
    rc = fn(*args)
    if rc != 0:
        raise RobirHipError(f"{name} failed ({rc}): {L.rb_last_error().decode()}")
