"""nn.Module mirrors of the reference's networks: identical constructor arguments and state-dict keys
(so Norm/Vis/PBR checkpoints load unchanged), forward passes run on the HIP kernels.

Mirrors: model/implicit_differentiable_renderer.py:170-258 (IndirctIllumNetwork, VisNetwork),
model/sg_envmap_material.py:40-275 (SparseAE, EnvmapMaterialNetwork),
model/neus_model.py:312-438,489-560,644-650,682-884 (SDFNetwork, RenderingNetwork, SingleVarianceNetwork,
NeuSModel, ImplicitNetworkMy).

Forward-only unless opted in: the network kernels carry no autograd.  A forward pass of a module that is in training mode, with grad enabled and
a parameter that requires grad, raises ForwardOnlyError (`forward_only_guard`; the drop-in is for inference /
--plot_only rendering) instead of handing detached outputs to a loss.  Material NETWORKS therefore still train on
the reference's modules; what IS differentiable on the HIP path is the SG shading of their outputs (robir_amd/sg_autograd.py,
sg_render.render_with_all_sg: light SGs, f0, roughness, albedo, metallic, indirect integral, predicted diffuse_vis) and -- after the explicit
opt-in robir_amd.training.enable_material_training -- the spec auto-encoder of EnvmapMaterialNetwork (robir_amd/ae_autograd.py), -- after
robir_amd.training.enable_visibility_training -- the visibility network (robir_amd/vis_autograd.py), and -- after
robir_amd.training.enable_illumination_training -- the indirect-illumination network (robir_amd/illum_autograd.py), and -- after
robir_amd.training.enable_cesr_training -- the CESR stage's shadow_net / normal_net (robir_amd/cesr_autograd.py).
Every forward that the reference randomises takes the draws as an optional explicit tensor (`noise=`); when omitted
they are drawn with torch.randn on the device, in the reference's order.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import dispatch, ops, packing
from .precision import cesr_precision, mlp_precision  # noqa: F401  ('f16x6' under the default policy, 'f16x3' under ROBIR_PRECISION=split)


class _Packed:
    """Lazy, parameter-version-keyed cache of packed weight blobs.  The Parameter objects of a module are looked up once
    (`.to()`, `load_state_dict` and optimiser steps change them in place: new storage / bumped version, same object);
    walking the module tree on every call cost ~10 % of a per-chunk forward()."""

    def __init__(self):
        self._cache = {}
        self._params = {}

    def blob(self, key, module, table, **more):
        """The packed blob `key` of `module`: table[key] = (packing function by name -- looked up when it packs -- or a callable, state-dict
        prefix, extra keyword arguments of the packer); more: keyword arguments known per instance only."""
        params = self._params.get(id(module))
        if params is None:
            params = self._params[id(module)] = list(module.parameters())
        sig = (tuple((p.data_ptr(), p._version) for p in params), params[0].device)
        ent = self._cache.get(key)
        if ent is None or ent[0] != sig:
            packer, prefix, kw = table[key]
            fn = packer if callable(packer) else getattr(packing, packer)
            sd = {prefix + k: v.detach() for k, v in module.state_dict(prefix="").items()}
            ent = self._cache[key] = (sig, fn(sd, device=params[0].device, **kw, **more))
        return ent[1]


def _blob_alias(key, sdf_only=None):
    """The accessor names that tools and tests use: packed_*() is _blob(key), packed_*(full=False) of the SDF network _blob(sdf_only)."""
    return lambda self, full=True: self._blob(key if full or sdf_only is None else sdf_only)


def _h3(route):
    """The scale_log2 argument of the split-precision kernels, for the routes that take one."""
    return {"scale_log2": packing.H3_SCALE_LOG2} if route.scale_log2 else {}


class ForwardOnlyError(RuntimeError):
    pass


PRECISE_GRAD_SPLIT = os.environ.get("ROBIR_PRECISE_GRAD", "split") == "split"      # "jvp": value and gradient in one f32-input pass (round 3)


def forward_only_guard(module):
    """The HIP kernels have no backward: a training-mode call that autograd would have to differentiate must not silently
    return detached tensors (loss.backward() would then train only whatever still carries a graph).  A module marked by
    robir_amd.training.enable_material_training (or, a VisNetwork, by enable_visibility_training; an IndirctIllumNetwork, by
    enable_illumination_training; an SDFNetwork of kind shadow / normal, by enable_cesr_training) has a backward and passes; its unmarked
    sub-networks still raise."""
    if (getattr(module, "_material_training", False) or getattr(module, "_visibility_training", False)
            or getattr(module, "_illumination_training", False) or getattr(module, "_cesr_training", False)):
        return
    if module.training and torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise ForwardOnlyError(f"{type(module).__name__}: robir_amd kernels are forward-only -- call .eval(), wrap the call in "
                               "torch.no_grad(), or freeze the parameters (training stays on the reference's modules)")


# ----------------------------------------------------------------------------------------- small-batch concurrency
# A single 1024-pixel chunk gives the 512-wide nets ~660 rows = 11 workgroups per launch: each launch is one workgroup's
# latency (0.12 ms) on a machine with 256 CUs, and a chunk runs five of them back to back.  Independent nets of one forward
# are therefore issued on side streams when the batch is small (joined before anything consumes them).  Whole-view batches
# fill the GPU by themselves and stay on the caller's stream.
SIDE_STREAMS = os.environ.get("ROBIR_SIDE_STREAMS", "1") != "0"
SIDE_STREAM_MAX_ROWS = 8192
BORROW_SLAB_ROWS = int(os.environ.get("ROBIR_BORROW_SLAB_ROWS", "65536"))     # rays per borrow_color slab (NeuSRenderer.batch_borrow_color)
_SIDE_POOL = {}


def run_concurrently(thunks, rows):
    """[t() for t in thunks]; for small batches on a GPU each thunk after the first runs on its own side stream.  Safe without
    record_stream bookkeeping: a side section starts only after an event recorded on the caller's stream (everything enqueued
    before -- including the consumers of tensors a previous side section allocated -- precedes it), and the caller's stream
    waits for every side stream before this function returns."""
    if len(thunks) < 2 or not SIDE_STREAMS or rows > SIDE_STREAM_MAX_ROWS or not torch.cuda.is_available():
        return [t() for t in thunks]
    cur = torch.cuda.current_stream()
    pool = _SIDE_POOL.get(cur.device)
    if pool is None:
        pool = _SIDE_POOL[cur.device] = [torch.cuda.Stream(device=cur.device) for _ in range(3)]
    ev = cur.record_event()
    outs = [None] * len(thunks)
    used = []
    for i in range(1, len(thunks)):
        st = pool[(i - 1) % len(pool)]
        st.wait_event(ev)
        with torch.cuda.stream(st):
            outs[i] = thunks[i]()
        used.append(st)
    outs[0] = thunks[0]()
    for st in used:
        cur.wait_stream(st)
    return outs


def _require_dims(name, got, want):
    if list(got) != list(want):
        raise NotImplementedError(f"{name}: the HIP kernels are built for dims {want}, got {list(got)}")


def _mlp(dim, dims, n_out, act):
    """nn.Sequential of Linear + act() per entry of dims and a last Linear to n_out (the reference's layer lists, same state-dict keys)."""
    layers = []
    for d in dims:
        layers += [nn.Linear(dim, d), act()]
        dim = d
    return nn.Sequential(*layers, nn.Linear(dim, n_out))


# ----------------------------------------------------------------------------------------- visibility
class VisNetwork(nn.Module):
    """implicit_differentiable_renderer.py:225-258."""

    def __init__(self, points_multires=10, dirs_multires=4, dims=[128, 128, 128, 128]):
        super().__init__()
        if points_multires != 10 or dirs_multires != 10:
            raise NotImplementedError("HIP visibility kernels are built for points_multires = dirs_multires = 10")
        _require_dims("visibility_network", dims, [256] * 4)
        self.vis_layer = _mlp(126, dims, 2, nn.ReLU)
        self._packed = _Packed()

    _BLOBS = {"full": ("pack_vis", "visibility_network.", {}), "full_h3": ("pack_vis_h3", "visibility_network.", {}),
              "full_x6": ("pack_vis_x6", "visibility_network.", {}), "split": ("pack_vis_split", "visibility_network.", {})}

    def _blob(self, key):
        return self._packed.blob(key, self, self._BLOBS)

    packed_full, packed_full_h3, packed_full_x6, packed_split = (_blob_alias(k) for k in ("full", "full_h3", "full_x6", "split"))

    def _trainable(self):
        """Marked by robir_amd.training.enable_visibility_training, grad mode on, a parameter that requires grad: calls build a graph."""
        return (getattr(self, "_visibility_training", False) and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def logits_from_features(self, X):
        """X [M,128] = [PE10(p) | PE10(d)] (ops.feat_vis) -> logits [M,2]; arithmetic per robir_amd.MLP_PRECISION."""
        forward_only_guard(self)
        if self._trainable():
            raise NotImplementedError("VisNetwork.logits_from_features: the HIP backward of the visibility network encodes the points and the "
                                      "directions itself (fp64 from the fp32 coordinates) -- call logits_from_points / forward while the network "
                                      "is marked by enable_visibility_training, or wrap the feature-row call in torch.no_grad()")
        r = dispatch.vis_mlp(mlp_precision(), ops.SDF_FUSED_PE, points=False)
        return getattr(ops, r.fn)(X, self._blob(r.blob), **_h3(r))

    def logits_from_points(self, points, dirs, rep=1):
        """points [M/rep,3], dirs [M,3] (rep consecutive directions per point) -> logits [M,2]: [PE10(p) | PE10(d)] is encoded
        inside the MLP kernel (no feature rows) unless ROBIR_SDF_FUSED_PE=0."""
        forward_only_guard(self)
        if self._trainable():
            from . import vis_autograd
            return vis_autograd.logits(self, points, dirs, rep)
        r = dispatch.vis_mlp(mlp_precision(), ops.SDF_FUSED_PE, points=True)
        if r.encode:
            return self.logits_from_features(ops.feat_vis(points.float().contiguous(), dirs.float().contiguous(), rep=rep))
        return getattr(ops, r.fn)(points, dirs, self._blob(r.blob), rep, **_h3(r))

    def forward(self, points, view_dirs):
        forward_only_guard(self)
        if points.shape[0] == 0:
            return torch.zeros(0, 2, device=points.device)
        return self.logits_from_points(points.float().contiguous(), view_dirs.float().contiguous())


# ----------------------------------------------------------------------------------------- sparse auto-encoder
class SparseAE(nn.Module):
    """sg_envmap_material.py:40-118 (forward/encode)."""

    def __init__(self, in_dim, out_dim, smooth_on_latent=True, out_act=torch.sigmoid, latent_dim=32, high_lr=False):
        super().__init__()
        if latent_dim != 32 or in_dim > 64 or out_dim > 16:
            raise NotImplementedError("HIP SparseAE kernels: in_dim <= 64, latent 32, out_dim <= 16")
        self.brdf_encoder_layer = _mlp(in_dim, [512] * 4, latent_dim, lambda: nn.LeakyReLU(0.2))
        self.brdf_decoder_layer = _mlp(latent_dim, [128, 128], out_dim, lambda: nn.LeakyReLU(0.2))
        self.in_dim, self.out_dim, self.latent_dim = in_dim, out_dim, latent_dim
        self.smooth_on_latent = smooth_on_latent
        self.out_act = out_act
        self.high_lr = high_lr
        self.lc_act = torch.sigmoid            # runners replace this with F.softplus for the integral layer
        self.var = torch.zeros(latent_dim)     # plain attribute, like the reference (not in the state dict)
        self._packed = _Packed()

    _BLOBS = {"ae": ("pack_sparse_ae", "ae.", {"prefix": "ae"}), "enc_h3": ("pack_sparse_ae_encoder_h3", "ae.", {"prefix": "ae"}),
              "enc_x6": ("pack_sparse_ae_encoder_x6", "ae.", {"prefix": "ae"})}

    def _blob(self, key):
        b = self._packed.blob(key, self, self._BLOBS)
        return b[0] if key == "ae" else b          # pack_sparse_ae: (encoder, decoder)

    def _blobs(self):
        return self._packed.blob("ae", self, self._BLOBS)

    def _encode(self, X):
        r = dispatch.wide(mlp_precision(), ops.SDF_FUSED_PE, points=False, encoder=True)
        return getattr(ops, r.fn)(X, self._blob(r.blob), *((True,) if r.flag else ()), **_h3(r))

    def _encode_points(self, pts):
        """_encode(feat_pe10(pts)) with the encoding fused into the encoder kernel unless ROBIR_SDF_FUSED_PE=0."""
        r = dispatch.wide(mlp_precision(), ops.SDF_FUSED_PE, points=True, encoder=True)
        if r.encode:
            return self._encode(ops.feat_pe10(pts))
        return getattr(ops, r.fn)(pts, None, self._blob(r.blob), True, **_h3(r))

    def run_points(self, pts, noise):
        """run(feat_pe10(pts), noise=noise) for latent-smoothed auto-encoders, straight from the points."""
        forward_only_guard(self)
        assert self.smooth_on_latent
        enc, dec = self._blobs()
        sig_out = self._sigmoid_out()
        lat, lat2 = ops.ae_latent(self._encode_points(pts), self._var(pts.device), self._latent_act_code(), noise, 0.01)
        return ops.ae_decode(lat, dec, self.out_dim, sig_out), ops.ae_decode(lat2, dec, self.out_dim, sig_out)

    def _sigmoid_out(self):
        if self.out_act is not None and getattr(self.out_act, "__name__", "") != "sigmoid":
            raise NotImplementedError("out_act must be torch.sigmoid or None")
        return self.out_act is not None

    def _trainable(self):
        """Marked by robir_amd.training.enable_material_training, grad mode on, a parameter that requires grad: calls build a graph."""
        return (getattr(self, "_material_training", False) and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def _latent_act_code(self):
        name = getattr(self.lc_act, "__name__", "")
        if name == "softplus":
            return 1
        if name == "sigmoid":
            return 0
        raise NotImplementedError(f"latent activation {self.lc_act}")

    def _var(self, dev):
        v = self.var
        if isinstance(v, torch.Tensor) and bool((v != 0).any()):
            return v.to(device=dev, dtype=torch.float32).contiguous()
        return None

    def run(self, X, noise=None, X_noisy=None, need_first=True):
        """X [n,64] padded features.  smooth_on_latent: noise [n,32]; else X_noisy [n,64] = features of the perturbed input.
        need_first=False skips the un-perturbed pass (the indirect-illumination integral only uses the second output)."""
        forward_only_guard(self)
        enc, dec = self._blobs()
        dev = X.device
        sig_out = self._sigmoid_out()
        if self.smooth_on_latent:
            lat, lat2 = ops.ae_latent(self._encode(X), self._var(dev), self._latent_act_code(), noise, 0.01)
        else:
            lat2, _ = ops.ae_latent(self._encode(X_noisy), self._var(dev), self._latent_act_code())
            if not need_first:
                return None, ops.ae_decode(lat2, dec, self.out_dim, sig_out)
            lat, _ = ops.ae_latent(self._encode(X), self._var(dev), self._latent_act_code())
        return ops.ae_decode(lat, dec, self.out_dim, sig_out), ops.ae_decode(lat2, dec, self.out_dim, sig_out)

    def run_pass(self, X):
        """One encode -> latent activation -> decode pass on features X [n,64] (no latent noise)."""
        forward_only_guard(self)
        enc, dec = self._blobs()
        lat, _ = ops.ae_latent(self._encode(X), self._var(X.device), self._latent_act_code())
        return ops.ae_decode(lat, dec, self.out_dim, self.out_act is not None)

    def encode(self, values):
        """sg_envmap_material.py:96-99: encoder output * (1 - var) on already-embedded rows [n, in_dim] (the pre-activation latent)."""
        forward_only_guard(self)
        flat = values.reshape(-1, values.shape[-1]).float()
        X = torch.zeros(flat.shape[0], 64, device=flat.device)
        X[:, :self.in_dim] = flat.detach()
        if self._trainable():
            from . import ae_autograd
            ae_autograd.refuse_input_grad(values=values)
            return ae_autograd.run_features(self, X)[2].reshape(list(values.shape[:-1]) + [self.latent_dim])
        raw, _ = ops.ae_latent(self._encode(X), self._var(flat.device), 2)
        return raw.reshape(list(values.shape[:-1]) + [self.latent_dim])

    def kl_divergence(self, rho, rho_hat):
        raise NotImplementedError("SparseAE.kl_divergence: a training loss term (model/sg_envmap_material.py:101-105; callers model/loss.py) -- "
                                  "losses are OUT OF SCOPE for the forward renderer (SURVEY.md section 2 row 9)")

    def kl_smooth_loss(self, points, kl_w, smooth_w):
        raise NotImplementedError("SparseAE.kl_smooth_loss: a training loss term (model/sg_envmap_material.py:107-118) -- losses are OUT OF "
                                  "SCOPE for the forward renderer (SURVEY.md section 2 row 9)")

    def forward(self, points, noise=None):
        """points [n,in_dim]: already-embedded inputs (the reference's parameter name, sg_envmap_material.py:74)."""
        values = points
        n = values.shape[0]
        X = torch.zeros(n, 64, device=values.device)
        X[:, :self.in_dim] = values
        if self.smooth_on_latent:
            if noise is None:
                noise = torch.randn(n, 32, device=values.device)
            return self.run(X, noise=noise)
        if noise is None:
            noise = torch.randn(n, self.in_dim, device=values.device)
        Xn = torch.zeros(n, 64, device=values.device)
        Xn[:, :self.in_dim] = ops.axpy(values.contiguous(), noise.contiguous(), 0.02)
        return self.run(X, X_noisy=Xn)


# ----------------------------------------------------------------------------------------- indirect illumination
class IndirctIllumNetwork(nn.Module):
    """implicit_differentiable_renderer.py:170-222."""

    def __init__(self, multires=0, dims=[128, 128, 128, 128], num_lgt_sgs=24, no_hdr=False):
        super().__init__()
        if multires != 10 or num_lgt_sgs != 24:
            raise NotImplementedError("HIP indirect-illumination kernels: multires=10, 24 lobes")
        _require_dims("indirect_illum_network", dims, [512] * 4)
        self.num_lgt_sgs = num_lgt_sgs
        self.use_hdr = not no_hdr              # hdr_mode == -1: no hdr-shift input column (feature 63 stays zero)
        in_dim = 64 if self.use_hdr else 63
        self.lobe_layer = _mlp(in_dim, dims, num_lgt_sgs * 6, nn.ReLU)
        self.integral_layer = SparseAE(in_dim, 3, out_act=None, smooth_on_latent=False)
        self.integral_layer.lc_act = torch.nn.functional.softplus
        self._packed = _Packed()

    _BLOBS = {"lobe": ("pack_illum", "indirect_illum_network.lobe_layer.", {}), "lobe_h3": ("pack_illum_h3", "indirect_illum_network.lobe_layer.", {}),
              "lobe_x6": ("pack_illum_x6", "indirect_illum_network.lobe_layer.", {})}

    def _trainable(self):
        """Marked by robir_amd.training.enable_illumination_training, grad mode on, a parameter that requires grad: calls build a graph."""
        return (getattr(self, "_illumination_training", False) and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def _lobes(self, points, hdr, X=None):
        """lgt_sgs [n,24,7] of points [n,3] and hdr [n,1] (None: no_hdr) under the current precision policy; X: their feature rows, if at hand."""
        r = dispatch.wide(mlp_precision(), ops.SDF_FUSED_PE, points=True, encoder=False)
        blob = self._packed.blob(r.blob, self.lobe_layer, self._BLOBS)
        if r.encode:        # feature rows; else [PE10(x) | hdr_shift] encoded inside the lobe net's kernel
            if X is None:
                X = ops.feat_pe10(points, extra=hdr)
            return ops.illum_decode(getattr(ops, r.fn)(X, blob, *((False,) if r.flag else ()), **_h3(r)))
        return ops.illum_decode(getattr(ops, r.fn)(points, hdr, blob, False, **_h3(r)))

    def _integral(self, X, noise):
        """env_int [n,3]: only the perturbed pass is used (implicit_differentiable_renderer.py:220)."""
        return ops.abs_scale(self.integral_layer.run_pass(ops.axpy(X, noise, 0.02)), 1.0)

    def forward(self, points, hdr_shift, noise=None):
        forward_only_guard(self)
        n = points.shape[0]
        dev = points.device
        if noise is None:
            noise = torch.randn(n, 64, device=dev)
        elif noise.shape[1] < 64:                # no_hdr: the reference draws randn_like of the 63 embedded columns
            noise = torch.nn.functional.pad(noise, (0, 64 - noise.shape[1]))
        if self._trainable():
            from . import illum_autograd
            return illum_autograd.forward(self, points, hdr_shift, noise)
        points = points.float().contiguous()
        hdr = hdr_shift.float().contiguous() if self.use_hdr else None
        X = ops.feat_pe10(points, extra=hdr)
        noise = noise.float().contiguous()
        sgs, integ = run_concurrently([lambda: self._lobes(points, hdr, X), lambda: self._integral(X, noise)], n)      # two independent nets
        return sgs, integ


# ----------------------------------------------------------------------------------------- materials + light
def fibonacci_sphere(samples=1):
    from .synth import fibonacci_lobes
    return fibonacci_lobes(samples).astype(np.float64)


def compute_energy(lgtSGs):
    lam = torch.abs(lgtSGs[:, 3:4])
    mu = torch.abs(lgtSGs[:, 4:])
    return mu * 2.0 * np.pi / lam * (1.0 - torch.exp(-2.0 * lam))


class EnvmapMaterialNetwork(nn.Module):
    """sg_envmap_material.py:121-275."""

    def __init__(self, multires=0, brdf_encoder_dims=[512, 512, 512, 512], brdf_decoder_dims=[128, 128],
                 num_lgt_sgs=32, upper_hemi=False, specular_albedo=0.02, latent_dim=32):
        super().__init__()
        if multires != 10:
            raise NotImplementedError("HIP material kernels: multires=10")
        self.numLgtSGs = num_lgt_sgs
        self.envmap = None
        self.latent_dim = latent_dim
        self.brdf_encoder_layer = SparseAE(63, 5, out_act=None)
        self.spec_brdf_encoder_layer = SparseAE(63, 5, high_lr=True)
        self.normal_decoder_layer = SparseAE(60, 3, out_act=None, smooth_on_latent=False)
        self.specular_reflectance = nn.Parameter(torch.full((1, 1), float(specular_albedo)))
        from .synth import synth_light_sgs
        self.lgtSGs = nn.Parameter(torch.from_numpy(synth_light_sgs(0, num_lgt_sgs)))
        self.upper_hemi = upper_hemi

    def restrict_lobes_upper(self, lgtSGs):
        return torch.cat((lgtSGs[..., :1], torch.abs(lgtSGs[..., 1:2]), lgtSGs[..., 2:]), dim=-1)

    def forward(self, points, train_spec=False, train_norm=False, noise=None):
        """noise: dict with optional 'spec' [n,32] and 'normal' [n,60]."""
        forward_only_guard(self)
        noise = noise or {}
        n, dev = points.shape[0], points.device
        pts = points.float().contiguous()
        nz_n = noise.get("normal")
        want_spec = train_norm is False or train_spec
        nz_s = None
        if want_spec:
            nz_s = noise.get("spec")
            if nz_s is None:
                nz_s = torch.randn(n, 32, device=dev)
            nz_s = nz_s.float().contiguous()
        if nz_n is None:
            nz_n = torch.randn(n, 60, device=dev)
        nz_n = nz_n.float().contiguous()
        # the spec auto-encoder and the two passes of the normal auto-encoder (clean / perturbed input) are independent
        thunks = [lambda: ops.normalize3(self.normal_decoder_layer.run_pass(ops.feat_ipe(pts, 1e-5)), 1e-4, 1),
                  lambda: ops.normalize3(self.normal_decoder_layer.run_pass(ops.feat_ipe(pts, 1e-5, nz_n, 0.02)), 1e-4, 1)]
        if want_spec:
            thunks.append(lambda: self.spec_brdf_encoder_layer.run_points(pts, nz_s))
        trainable = (getattr(self, "_material_training", False) and torch.is_grad_enabled()
                     and any(p.requires_grad for p in self.parameters()))
        if trainable:
            # robir_amd.training: the spec auto-encoder carries a graph and runs on the caller's stream; the normal decoder has no backward
            # (no stage-3 loss term reaches it) and runs without one
            from . import ae_autograd
            ae_autograd.refuse_input_grad(points=points)
            with torch.no_grad():
                res = run_concurrently(thunks[:2], n)
            if want_spec:
                ae = self.spec_brdf_encoder_layer
                if ae._trainable():
                    brdf, brdf_r, _ = ae_autograd.run_points(ae, pts, nz_s)
                else:
                    with torch.no_grad():
                        brdf, brdf_r = ae.run_points(pts, nz_s)
                if not train_spec:                # the reference's .detach() (model/sg_envmap_material.py:196)
                    brdf, brdf_r = brdf.detach(), brdf_r.detach()
                res = list(res) + [(brdf, brdf_r)]
        else:
            res = run_concurrently(thunks, n)
        normal_map, random_xi_normal = res[0], res[1]
        if want_spec:
            brdf, brdf_r = res[2]
        if train_norm:
            return {"sg_normal_map": normal_map, "random_xi_normal": random_xi_normal}
        lgtSGs = self.restrict_lobes_upper(self.lgtSGs) if self.upper_hemi else self.lgtSGs
        if trainable and (brdf.requires_grad or brdf_r.requires_grad):
            alb, rough, metal, alb_r, rough_r, metal_r = ae_autograd.material_decode(brdf, brdf_r)
        else:
            alb, rough, metal, alb_r, rough_r, metal_r = ops.material_decode(brdf, brdf_r)
        return {
            "sg_lgtSGs": lgtSGs,
            "sg_specular_reflectance": self.specular_reflectance,
            "sg_roughness": rough,
            "sg_metallic": metal,
            "sg_normal_map": normal_map,
            "sg_diffuse_albedo": alb,
            "random_xi_roughness": rough_r,
            "random_xi_metallic": metal_r,
            "random_xi_diffuse_albedo": alb_r,
            "random_xi_normal": random_xi_normal,
        }

    def get_light(self):
        lgtSGs = self.lgtSGs.clone().detach()
        return self.restrict_lobes_upper(lgtSGs) if self.upper_hemi else lgtSGs

    def load_light(self, path):
        """sg_envmap_material.py:257-268: `<path>/sg_128.npy` light SGs + `<path>.exr` background map (read by robir_amd.exr:
        the reference goes through imageio)."""
        from . import deferred
        deferred.flush_all()               # recorded chunk forwards were meant for the light that is loaded now
        sg = torch.from_numpy(np.load(os.path.join(path, "sg_128.npy"))).to(self.lgtSGs.data.device)
        self.lgtSGs.data = sg
        from .exr import read_exr
        self.envmap = torch.from_numpy(np.ascontiguousarray(read_exr(path + ".exr")[:, :, :3])).to(sg.device)

    def parameter_groups(self, lr=0.0005):
        return [{"lr": lr, "params": self.brdf_encoder_layer.parameters()},
                {"lr": lr, "params": self.spec_brdf_encoder_layer.parameters()},
                {"lr": lr, "params": self.normal_decoder_layer.parameters()},
                {"lr": lr, "params": self.specular_reflectance},
                {"lr": lr, "params": self.lgtSGs}]


# ----------------------------------------------------------------------------------------- NeuS networks
def _wn_linear(k_in, n_out):
    return nn.utils.weight_norm(nn.Linear(k_in, n_out))


def _pack_sdf_back_x6(sd, device):
    """ops.sdf_value_grad_x6's `back`: the one-tile kernel's transposed layers, the head row, the two-tile kernel's transposed layers."""
    wt, w8 = packing.pack_sdf_back_x6(sd, device)
    return wt, w8, packing.pack_sdf_back_x6(sd, device, two_tile=True)[0]


class SDFNetwork(nn.Module):
    """neus_model.py:312-438.  Three shapes are compiled:
      (d_in 3,   d_out 257, 256 x 8, skip [4], multires 10)  -- the NeuS SDF network (default arguments)
      (d_in 63,  d_out 3,   512 x 8, skip [4], multires 0)   -- CESR normal_net  (training/train_cesr.py:109)
      (d_in 191, d_out 2,   512 x 8, skip [4], multires 0)   -- CESR shadow_net  (training/train_cesr.py:107)"""

    def __init__(self, d_in, d_out, d_hidden, n_layers, skip_in=(4,), multires=10, bias=0.5, scale=1,
                 geometric_init=True, weight_norm=True, inside_outside=False, embed="Default"):
        super().__init__()
        if multires > 0 and embed == "IPE":
            raise NotImplementedError("SDFNetwork(embed='IPE'): the HIP SDF kernels encode with PE (every shipped configuration sets "
                                      "ENCODING = 'PE', confs_sg/env_path.py:5); the IPE-SDF variant is OUT OF SCOPE (SURVEY.md section 2 row 2)")
        key = (d_in, d_out, d_hidden, n_layers, tuple(skip_in), multires)
        kinds = {(3, 257, 256, 8, (4,), 10): "neus", (63, 3, 512, 8, (4,), 0): "normal", (191, 2, 512, 8, (4,), 0): "shadow"}
        if key not in kinds or not weight_norm or scale != 1:
            raise NotImplementedError(f"SDFNetwork{key}: the HIP kernels are compiled for {list(kinds)}")
        self.kind = kinds[key]
        self.d_in = d_in
        first = 63 if self.kind == "neus" else d_in
        dims = [first] + [d_hidden] * n_layers + [d_out]
        for l in range(n_layers + 1):
            out = dims[l + 1] - dims[0] if l + 1 in skip_in else dims[l + 1]
            setattr(self, "lin%d" % l, _wn_linear(dims[l], out))
        self.scale = 1
        self._packed = _Packed()

    _SDF = "implicit_network.neus_model.sdf_network."
    _BLOBS = {"full": ("pack_sdf", _SDF, {"full": True}), "sdf": ("pack_sdf", _SDF, {"full": False}),
              "full_h3": ("pack_sdf_h3", _SDF, {"full": True}), "sdf_h3": ("pack_sdf_h3", _SDF, {"full": False}),
              "x6_full": ("pack_sdf_x6", _SDF, {"full": True}), "x6_dist": ("pack_sdf_x6", _SDF, {"full": False}),
              "back": ("pack_sdf_back", _SDF, {}), "back_h3": ("pack_sdf_back_h3", _SDF, {}), "back_x6": (_pack_sdf_back_x6, _SDF, {})}
    _BLOBS_512 = {"w512": ("pack_softplus512", "net.", {"prefix": "net."}), "w512_h3": ("pack_softplus512_h3", "net.", {"prefix": "net."}),
                  "w512_x6": ("pack_softplus512_x6", "net.", {"prefix": "net."}), "w512_f16": ("pack_softplus512_f16", "net.", {"prefix": "net."})}

    def _blob(self, key):
        if self.kind == "neus":
            return self._packed.blob(key, self, self._BLOBS)
        return self._packed.blob(key, self, self._BLOBS_512, k_in=self.d_in)

    def packed(self, full=True):
        return self._blob(("full" if full else "sdf") if self.kind == "neus" else "w512")

    packed_h3, packed_x6 = _blob_alias("full_h3", "sdf_h3"), _blob_alias("x6_full", "x6_dist")
    packed_back, packed_back_h3, packed_back_x6, packed_w512_h3 = (_blob_alias(k) for k in ("back", "back_h3", "back_x6", "w512_h3"))

    def eval_points(self, x, in_scale=1.0, out_scale=1.0, full=True, grad=False, precise=False):
        """NeuS shape only.  x [M,3] -> (out [M,257] | [M], grad [M,3] | None); grad = d(out_scale*sdf(in_scale*x))/dx.
        precise: library-grade softplus (expf / log1pf on the f32-input MFMA, sdf-only modes) for VALUES that feed exact threshold
        decisions (the octree build).  With grad=True under the default policy the flag covers the value only: the gradient comes from
        the exact-operand reverse pass (ROBIR_PRECISE_GRAD=split, the default), whose softplus is the hardware-transcendental form.
        The kernel(s) that serve the call: dispatch.sdf."""
        assert self.kind == "neus"
        forward_only_guard(self)
        x = x.float().contiguous()
        M = x.shape[0]
        route = dispatch.sdf(full, grad, precise, M, mlp_precision(), ops.SDF_FUSED_PE, ops.SDF_KERNEL, ops.SDF_GRAD, PRECISE_GRAD_SPLIT,
                             ops.sdf_ring_waves, ops.SDF_GRAD_MIN_POINTS, ops.SDF_GRAD_F32_MIN_POINTS)
        scale = {"i": in_scale, "o": out_scale, "g": out_scale * in_scale}
        res = []
        for c in route.calls:
            args = [ops.feat_pe10(x, scale=in_scale, jvp=grad) if c.rows else x, M]
            args += [self._packed.blob(k, self, self._BLOBS) for k in c.blobs]
            args += c.sel
            if c.scale_log2:
                args.append(packing.H3_SCALE_LOG2)
            res.append(getattr(ops, c.fn)(*args, *[scale[k] for k in c.scales]))
        if route.combine == "precise":
            return res[0][0], res[1][1]
        if route.combine == "value":
            return res[0], None
        out, g = res[0]
        return (out[:, 0].contiguous() if route.combine == "column" else out), g

    def _cesr_route(self, r, x, M, kind, n_label):
        return getattr(ops, r.fn)(x, M, kind, self._blob(r.blob), n_label=n_label, **_h3(r))

    def _trainable(self):
        """Marked by robir_amd.training.enable_cesr_training, grad mode on, a parameter that requires grad: calls build a graph."""
        return (getattr(self, "_cesr_training", False) and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def _cesr_eval(self, x, M, kind, n_label, points):
        """The forward-only route of the current policy: on points (encoding inside the kernel, whatever ROBIR_SDF_FUSED_PE says) or on rows."""
        r = dispatch.cesr(mlp_precision(), cesr_precision(), True if points else ops.SDF_FUSED_PE, points=points)
        return self._cesr_route(r, x, M, kind, n_label)

    def _cesr_head(self, x, M, kind, n_label, points, head):
        """head 0: the raw output; 1: ops.softmax2(., 1); 2: ops.normalize3(., 1e-4, 1).  Through robir_amd/cesr_autograd.py when trainable."""
        forward_only_guard(self)
        if self._trainable():
            from . import cesr_autograd
            return cesr_autograd.apply(self, x, M, kind, n_label, points, head)
        from .cesr_autograd import HEADS
        return HEADS[head](self._cesr_eval(x, M, kind, n_label, points))

    def _cesr(self, X, M, kind, n_label=1):
        return self._cesr_head(X, M, kind, n_label, False, 0)

    def _cesr_points(self, pts, M, kind, n_label=1):
        """_cesr on PE10(pts) with the encoding evaluated inside the kernel (kind 0 normal_net, 2 shadow_net x labels), whatever
        ROBIR_SDF_FUSED_PE says: a caller that honours it asks dispatch.cesr itself (renderer.CESRHook)."""
        return self._cesr_head(pts, M, kind, n_label, True, 0)

    def eval_point_labels(self, Xp, n_label=128):
        """shadow_net on every (point, one-hot label) pair: Xp [n,64] PE10 features, or the points [n,3] themselves (encoded inside the
        kernel) -> logits [n*n_label, 2]."""
        assert self.kind == "shadow"
        return self._cesr_head(Xp, Xp.shape[0] * n_label, 2, n_label, Xp.shape[1] == 3, 0)

    def diffuse_vis(self, Xp, n_label=128):
        """shadow_net's predicted visibility of every (point, label) pair, ops.softmax2(eval_point_labels(Xp, n_label), 1) [n*n_label]: with
        a graph to the network's parameters when it is trainable (cesr_autograd.VisFn); forward-only it IS that expression."""
        assert self.kind == "shadow"
        if self._trainable():
            return self._cesr_head(Xp, Xp.shape[0] * n_label, 2, n_label, Xp.shape[1] == 3, 1)
        return ops.softmax2(self.eval_point_labels(Xp, n_label), 1)

    def unit_normal(self, Xp):
        """normal_net's unit normal, ops.normalize3(raw, 1e-4, 1) [n,3], of PE10 features [n,64] or points [n,3]: with a graph to the
        network's parameters when it is trainable (cesr_autograd.UnitFn)."""
        assert self.kind == "normal"
        return self._cesr_head(Xp, Xp.shape[0], 0, 1, Xp.shape[1] == 3, 2)

    def forward(self, inputs, var=0.0001, chunk=1024):
        if inputs.numel() == 0:
            return torch.ones_like(inputs)
        shape = list(inputs.shape[:-1]) + [-1]
        if self.kind == "neus":
            out, _ = self.eval_points(inputs.reshape(-1, 3))
            return out.reshape(shape)
        flat = inputs.reshape(-1, self.d_in).float()
        M = flat.shape[0]
        kp = 64 if self.kind == "normal" else 192
        X = torch.zeros(M, kp, device=flat.device)
        X[:, :self.d_in] = flat
        return self._cesr(X, M, 0 if self.kind == "normal" else 1).reshape(shape)

    def sdf(self, x):
        assert self.kind == "neus"
        out, _ = self.eval_points(x.reshape(-1, 3), full=False)
        return out[:, None]

    def sdf_hidden_appearance(self, x):
        return self.forward(x)

    def gradient(self, x):
        assert self.kind == "neus"
        _, g = self.eval_points(x.reshape(-1, 3), full=False, grad=True)
        return g.unsqueeze(1)


class RenderingNetwork(nn.Module):
    """neus_model.py:489-560, mode 'idr' (d_feature 256, d_hidden 256, 4 layers, multires_view 4)."""

    def __init__(self, d_feature, mode, d_in, d_out, d_hidden, n_layers, weight_norm=True, multires_view=4, squeeze_out=True):
        super().__init__()
        got = (d_feature, mode, d_in, d_out, d_hidden, n_layers, bool(weight_norm), multires_view, bool(squeeze_out))
        want = (256, "idr", 9, 3, 256, 4, True, 4, True)
        if got != want:
            raise NotImplementedError(f"RenderingNetwork{got}: the HIP colour kernels are compiled for {want} (what NeuSModel builds, "
                                      "model/neus_model.py:717-718)")
        self.mode, self.squeeze_out = mode, True
        dims = [289, 256, 256, 256, 256, 3]
        for l in range(5):
            setattr(self, "lin%d" % l, _wn_linear(dims[l], dims[l + 1]))
        self._packed = _Packed()

    _COL = "implicit_network.neus_model.color_network."
    _BLOBS = {"c": ("pack_color", _COL, {}), "c_x6": ("pack_color_x6", _COL, {}), "c_h3": ("pack_color_h3", _COL, {})}

    def _blob(self, key):
        return self._packed.blob(key, self, self._BLOBS)

    packed, packed_x6, packed_h3 = (_blob_alias(k) for k in ("c", "c_x6", "c_h3"))

    def forward(self, points, normals, view_dirs, feature_vectors, x_scale=1.0, feat_scale=1.0):
        forward_only_guard(self)
        r = dispatch.color(mlp_precision(), ops.SDF_FUSED_PE)
        if r.encode:
            X = ops.feat_color(points.float().contiguous(), view_dirs.float().contiguous(), normals.float().contiguous(),
                               feature_vectors, x_scale=x_scale, feat_scale=feat_scale)
            return getattr(ops, r.fn)(X, self._blob(r.blob))
        return getattr(ops, r.fn)(points, view_dirs, normals, feature_vectors, self._blob(r.blob), **_h3(r), x_scale=x_scale, feat_scale=feat_scale)


class SingleVarianceNetwork(nn.Module):
    def __init__(self, init_val):
        super().__init__()
        self.register_parameter("variance", nn.Parameter(torch.tensor(init_val)))

    def forward(self, x):
        return torch.ones([len(x), 1], device=x.device) * torch.exp(self.variance * 10.0)


class HashSDFNetwork(nn.Module):
    def __init__(self, d_in, d_out, multires=12, dx_curve=0.1, separated=False):
        raise NotImplementedError("HashSDFNetwork: tinycudann hash-grid SDF, never instantiated (hashing=False, model/neus_model.py:774) -- "
                                  "OUT OF SCOPE (SURVEY.md section 2 row 2)")

    def forward(self, inputs):
        raise NotImplementedError("HashSDFNetwork is OUT OF SCOPE (SURVEY.md section 2 row 2)")

    def sdf(self, x):
        raise NotImplementedError("HashSDFNetwork is OUT OF SCOPE (SURVEY.md section 2 row 2)")

    def sdf_hidden_appearance(self, x):
        raise NotImplementedError("HashSDFNetwork is OUT OF SCOPE (SURVEY.md section 2 row 2)")

    def gradient(self, x, dx=None):
        raise NotImplementedError("HashSDFNetwork is OUT OF SCOPE (SURVEY.md section 2 row 2)")


class NeRF(nn.Module):
    def __init__(self, D=8, W=256, d_in=3, d_in_view=3, multires=10, multires_view=4, output_ch=4, skips=[4], use_viewdirs=True):
        raise NotImplementedError("NeRF: the NeRF++ outside-the-sphere background model, built only when NeuSModel(outside=True) -- no shipped "
                                  "configuration does (n_outside=0, neus/config/render.gin:12) -- OUT OF SCOPE (SURVEY.md section 2 rows 2, 6)")

    def forward(self, input_pts, input_views):
        raise NotImplementedError("NeRF is OUT OF SCOPE (SURVEY.md section 2 rows 2, 6)")


def auto_flatten(f):
    """neus_model.py:653-662: call `f(self, x [M,3], ...)` on the flattened points and give the result x's leading shape."""
    import functools

    @functools.wraps(f)
    def wrapper(self, x, *args, **kwargs):
        lead = list(x.shape[:-1])
        return f(self, x.reshape(-1, 3), *args, **kwargs).reshape(lead + [-1])
    return wrapper


def auto_flatten2(f):
    """neus_model.py:665-678: the two-output form for `f(self, x, dirs, ...) -> (rgb, a)`; dirs [R,3] broadcast over the samples of x [R,S,3]."""
    import functools

    @functools.wraps(f)
    def wrapper(self, x, dirs, *args, **kwargs):
        lead = list(x.shape[:-1])
        if len(lead) + 1 > dirs.dim():
            dirs = dirs[:, None, :].expand(x.shape)
        rgb, a = f(self, x.reshape(-1, 3), dirs.reshape(-1, 3), *args, **kwargs)
        return rgb.reshape(lead + [-1]), a.reshape(lead + [-1])
    return wrapper


class NeuSModel(nn.Module):
    """neus_model.py:682-752 (mode 'idr', hashing False, no outside NeRF)."""

    def __init__(self, mode="idr", hashing=False, outside=False, embed="IPE"):
        super().__init__()
        if mode != "idr" or hashing or outside or embed != "PE":
            raise NotImplementedError(f"NeuSModel(mode={mode!r}, hashing={hashing}, outside={outside}, embed={embed!r}): only the shipped NeuS "
                                      "configuration is built -- mode 'idr', no hash grid, no outside NeRF, embed='PE' (ImplicitNetworkMy passes "
                                      "confs_sg.env_path.ENCODING = 'PE', model/neus_model.py:771-776; the constructor's own default 'IPE' is not "
                                      "what any shipped checkpoint uses).  OUT OF SCOPE: SURVEY.md section 2 row 2")
        self.color_network = RenderingNetwork(d_feature=256, mode=mode, d_in=9, d_out=3, d_hidden=256, n_layers=4)
        self.sdf_network = SDFNetwork(d_in=3, d_out=257, d_hidden=256, n_layers=8, embed=embed)
        self.deviation_network = SingleVarianceNetwork(init_val=0.3)

    def sdf(self, x):
        return self.sdf_network.sdf(x)

    def sdf_and_feat(self, x):
        out = self.sdf_network(x)
        return out[..., :1], out[..., 1:]

    def color(self, x, gradients, dirs, feature_vector):
        return self.color_network(x, gradients, dirs, feature_vector)

    def grad(self, x):
        shape = list(x.shape[:-1]) + [-1]
        return self.sdf_network.gradient(x.reshape(-1, 3)).reshape(shape)

    def dev(self, x):
        return self.deviation_network(x)

    def radius(self):
        return 2.0

    def background(self, x, dirs):
        raise NotImplementedError("NeuSModel.background: the NeRF++ outside model is never built (outside=False, n_outside=0 in every "
                                  "configuration) -- OUT OF SCOPE (SURVEY.md section 2 rows 2, 6)")

    def inv_s(self):
        """exp(10 * variance) clipped to [1e-6, 1e6] as a host float.  Reading it is a device synchronisation, and borrow_color
        needs it for every 8192-point batch: cached on the parameter itself (same object, storage and version -- a real
        nn.Parameter, not a temporary).  Optimizer steps, load_state_dict and any in-place op on the parameter bump its version;
        a write through `variance.data` does not (autograd's escape hatch) -- call refresh_inv_s() after one."""
        v = self.deviation_network.variance
        key = (v.data_ptr(), v._version, v.device)
        if getattr(self, "_inv_s_key", None) != key:
            raw = float(torch.exp(v.detach() * 10.0))
            self._inv_s_raw = raw
            self._inv_s_val = min(max(raw, 1e-6), 1e6)
            self._inv_s_key = key
        return self._inv_s_val

    def inv_s_unclipped(self):
        """exp(10 * variance) as NormalTrainRunner.get_neus_surface uses it (no clip), from the same cache (no host read per call)."""
        self.inv_s()
        return self._inv_s_raw

    def refresh_inv_s(self):
        self._inv_s_key = None

    def forward(self, pnts, dirs, **kwargs):
        shape = list(pnts.shape[:-1]) + [-1]
        if len(shape) > dirs.dim():
            dirs = dirs[:, None, :].expand(pnts.shape)
        x, d = pnts.reshape(-1, 3), dirs.reshape(-1, 3)
        out, g = self.sdf_network.eval_points(x, full=True, grad=True)
        rgb = self.color_network(x, g, d, out[:, 1:])
        return rgb.view(shape), out[:, :1].reshape(shape)


def load_neus_checkpoint(neus_model, path):
    """Stage-1 checkpoint `{step:06d}.tar` = {'global_step', 'resume_time', 'model': state_dict, ...} written by
    neus/optimization/log.py:75-88, read like neus_model.py:779-781 (strict=False).  Keys of the three networks this
    build evaluates (sdf_network, color_network, deviation_network) must all be present; anything else the checkpoint
    carries (e.g. an outside-NeRF) is reported, not loaded."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    if "model" not in state:
        raise KeyError(f"{path}: no 'model' entry (found {sorted(state)}) -- not a NeuS stage-1 checkpoint")
    res = neus_model.load_state_dict(state["model"], strict=False)
    if res.missing_keys:
        raise KeyError(f"{path}: NeuS checkpoint lacks {len(res.missing_keys)} tensors of the SDF / colour / variance "
                       f"networks, e.g. {res.missing_keys[:4]}")
    if res.unexpected_keys:
        import warnings
        warnings.warn(f"{path}: {len(res.unexpected_keys)} tensors not used by this build "
                      f"(e.g. {res.unexpected_keys[:4]})", RuntimeWarning, stacklevel=2)
    return int(state.get("global_step", 0))


class ImplicitNetworkMy(nn.Module):
    """neus_model.py:755-884: stage-2 wrapper around the NeuS model (points x2 in, all 257 outputs /2 out).
    The constructor arguments of the conf (dims, multires, ...) are ignored exactly like the reference does; the NeuS
    checkpoint named by confs_sg.env_path is loaded when that module is importable and the file exists."""

    def __init__(self, feature_vector_size=None, d_in=None, d_out=None, dims=None, geometric_init=True, bias=1.0,
                 skip_in=(), weight_norm=True, multires=0, bgr=False):
        super().__init__()
        try:
            from confs_sg.env_path import NEUS_LOG_DIR, NEUS_ITER      # reference-side global (confs_sg/env_path.py)
            from confs_sg import env_path as _env
            encoding = getattr(_env, "ENCODING", "PE")
        except ImportError:
            NEUS_LOG_DIR = None
            encoding = "PE"
        self.neus_model = NeuSModel(mode="idr", hashing=False, embed=encoding)        # raises for anything but 'PE'
        self.bgr = bgr
        if NEUS_LOG_DIR is None:
            # stand-alone use (tests, bench, robir_amd.render): the caller loads the NeuS weights itself
            import warnings
            warnings.warn("ImplicitNetworkMy: confs_sg.env_path is not set up -- the NeuS SDF / colour networks keep their "
                          "random initialisation until a state dict is loaded", RuntimeWarning, stacklevel=2)
        else:
            # the reference raises here when the checkpoint is missing (neus_model.py:779); so do we -- a wrong
            # NEUS_LOG_DIR / NEUS_ITER must not silently render a randomly initialised surface
            path = os.path.join(NEUS_LOG_DIR, "{:06d}.tar".format(NEUS_ITER))
            if not os.path.exists(path):
                raise FileNotFoundError(f"NeuS checkpoint {path} (confs_sg.env_path) does not exist")
            load_neus_checkpoint(self.neus_model, path)

    def normalize(self, x):
        return x * 2.0

    def forward(self, points, compute_grad=False):
        if points.numel() == 0:
            return torch.ones_like(points)
        out, _ = self.neus_model.sdf_network.eval_points(points.reshape(-1, 3), 2.0, 0.5, full=True)
        return out

    def sdf_only(self, points):
        """[M] stage-2 signed distance (last layer restricted to its first row)."""
        return self.neus_model.sdf_network.eval_points(points.reshape(-1, 3), 2.0, 0.5, full=False)[0]

    def color(self, points, normals, view_dirs, feature_vectors):
        c = self.neus_model.color_network(points, normals, view_dirs, feature_vectors, x_scale=2.0)
        return c.flip(-1) if self.bgr else c

    def gradient(self, x):
        if x.numel() == 0:
            return torch.ones_like(x)
        _, g = self.neus_model.sdf_network.eval_points(x.reshape(-1, 3), 2.0, 0.5, full=False, grad=True)
        return g.unsqueeze(1)

    def get_parameter_groups(self, **lr_dict):
        res = []
        if "color" in lr_dict:
            res += [{"lr": lr_dict["color"], "params": self.neus_model.sdf_network.parameters()}]
        if "sdf" in lr_dict:
            res += [{"lr": lr_dict["sdf"], "params": self.neus_model.color_network.parameters()}]
        return res

    def volume_render(self, sdf, color):
        """sdf [m,ns,1], color [m,ns,3] -> [m,3] (neus_model.py:828-854)."""
        rgb, _ = ops.neus_composite(sdf.reshape(sdf.shape[0], -1).contiguous(), color.contiguous(),
                                    self.neus_model.inv_s())
        return rgb

    def borrow_color(self, points, view_dirs):
        tk = torch.linspace(-0.01, 0.05, 16).to(points.device)
        x, d = ops.borrow_points(points, view_dirs, tk)
        net = self.neus_model.sdf_network
        out, g = net.eval_points(x, 1.0, 1.0, full=True, grad=True)
        col = self.neus_model.color_network(x, g, d, out[:, 1:])
        m = points.shape[0]
        rgb, _ = ops.neus_composite(out[:, 0].reshape(m, 16).contiguous(), col.reshape(m, 16, 3), self.neus_model.inv_s())
        return rgb

    def batch_borrow_color(self, points, view_dirs, batch_size=None):
        """neus_model.py:873-884.  The reference walks the rays in batches of 8192 (its default) to bound ITS memory; the rows are
        independent (nothing batch-global), so with `batch_size` left at its default a batch here is a slab of BORROW_SLAB_ROWS rays (x 16
        samples: 1 M network evaluations, 1 GB of outputs + 9 GB of gradient scratch): a view's 3.4 M secondary hits in 53 slabs instead of
        420 batches x 3 kernels of 0.4-0.8 ms.  An explicit `batch_size` is honoured (a caller bounding memory).  Results are equal to fp32
        summation order whatever the batch size (the SDF / colour kernels pick their one- or two-tile form by launch size)."""
        if points.shape[0] == 0:
            return torch.zeros_like(points)
        step = BORROW_SLAB_ROWS if batch_size is None else max(1, int(batch_size))
        with torch.no_grad():
            outs = [self.borrow_color(points[i:i + step].contiguous(), view_dirs[i:i + step].contiguous())
                    for i in range(0, points.shape[0], step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


# ----------------------------------------------------------------------------------------- tone mapping
class ACESToneMapping(nn.Module):
    """color_correction.py:76-137: hdr_mode 0 scale_aces (every shipped conf), 1 warp_aces, 2 ln_space, else identity."""

    def __init__(self, hdr_mode=0):
        super().__init__()
        self.adapt_illum = nn.Parameter(torch.tensor(0.0))
        self.hdr_mode = hdr_mode
        self._curve = hdr_mode if hdr_mode in (0, 1, 2) else 3

    def as_input(self):
        return torch.clamp(self.adapt_illum * 10 + 0.5, 0, 1).view(1, 1)

    def make_shift(self, shift):
        if shift is None:
            shift = self.as_input()
        if not isinstance(shift, torch.Tensor):
            shift = torch.tensor(shift, device=self.adapt_illum.device)
        if shift.dim() == 0:
            shift = shift[None]
        return shift.detach().float()

    def _apply_tm(self, x, raw_shift, mode):
        shape = x.shape
        rows = x.numel() // 3
        p = self.adapt_illum
        from . import deferred
        if getattr(self, "_tonemap_training", False) and torch.is_grad_enabled() and not deferred.is_deferred(x):
            # robir_amd.training.enable_tonemap_training: the same bits with a graph to x, to a raw_shift tensor and -- raw_shift=None -- to
            # adapt_illum through as_input().  The cached shift below carries no graph: it neither serves nor is written by this branch.
            live = self.as_input() if raw_shift is None else raw_shift
            if x.requires_grad or (isinstance(live, torch.Tensor) and live.requires_grad):
                from . import tonemap_autograd
                if not isinstance(live, torch.Tensor):
                    live = torch.tensor(live, device=x.device)
                sh = live.float().reshape(-1).to(x.device)
                if sh.numel() != 1 and sh.numel() != rows:
                    raise ValueError(f"ACESToneMapping: a shift of {sh.numel()} values for {rows} rows (one value, or one per row)")
                return tonemap_autograd.tonemap(x.float().reshape(-1, 3), sh, self._curve, mode).reshape(shape)
        key = (p.data_ptr(), p._version, x.device)
        if raw_shift is None and getattr(self, "_shift_key", None) == key:
            sh = self._shift_val               # the model's own shift: ten tiny launches per call otherwise
        else:
            sh = self.make_shift(raw_shift).reshape(-1).to(x.device)
            if sh.numel() != 1 and sh.numel() != rows:
                sh = sh.expand(rows) if sh.numel() == 1 else sh.reshape(-1)
            sh = sh.contiguous()
            if raw_shift is None:
                self._shift_key, self._shift_val = key, sh
        from . import deferred

        def run(v):
            xs = v.detach().float().reshape(-1, 3).contiguous()
            return ops.tonemap(xs, sh, mode + 16 * self._curve).reshape(shape)
        if deferred.is_deferred(x):        # a recorded chunk forward (deferred.py): tone-map when its pass has run
            return deferred.lazy_like(x, run)
        return run(x)

    def hdr2ldr(self, x, raw_shift=None):
        return self._apply_tm(x, raw_shift, 0)

    def ldr2hdr(self, x, raw_shift=None):
        return self._apply_tm(x, raw_shift, 1)

    def fit_data(self, data):
        raise NotImplementedError("Energy.gen_cache is a training-time pre-fit (out of scope, SURVEY.md section 2 #9)")

    def plot(self, shift=1.0):
        raise NotImplementedError("ACESToneMapping.plot: a matplotlib debugging plot (model/color_correction.py:103-109) -- plots are OUT OF "
                                  "SCOPE (SURVEY.md section 2)")

    def scalar(self, shift):
        raise NotImplementedError("ACESToneMapping.scalar: reads the Energy cache that fit_data pre-fits at training time "
                                  "(model/color_correction.py:111-113, model/energy_integral.py) -- OUT OF SCOPE (SURVEY.md section 2 #9)")


class GammaCorrect(nn.Module):
    """color_correction.py:7-28."""

    def __init__(self, gamma=2.2, hdr_mode=0):
        super().__init__()
        self.gamma = nn.Parameter(torch.tensor(float(gamma)))
        self.indir_coef = nn.Parameter(torch.tensor(1.0))
        self.dir_coef = nn.Parameter(torch.tensor(2.0))
        self.coef = nn.Parameter(torch.tensor(1.0))
        self.hdr_shift = ACESToneMapping(hdr_mode=hdr_mode)

    def forward(self, x):
        return torch.pow(x, 1 / self.gamma)

    def inv(self, x):
        return torch.pow(x, self.gamma)
