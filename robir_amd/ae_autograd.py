"""Differentiable spec auto-encoder: a torch.autograd.Function around the forward kernels of nets.SparseAE and rb_train_ae_bwd.

Differentiable inputs: the sixteen nn.Linear tensors of ONE latent-smoothed SparseAE (smooth_on_latent=True).  The points / feature rows, the
latent noise and `var` are constants: a tensor that requires grad there raises NotImplementedError instead of receiving a silent zero.  The
forward runs the module's own forward kernels under the current precision policy -- its outputs are the forward-only path's, bit for bit -- and
returns (out, out_xi, raw_latent): the clean and the perturbed decoder output and the pre-activation latent (what SparseAE.encode returns, what
the KL term reads).  The backward is ONE call into the training library, which recomputes every activation in fp64 from the fp32 feature rows
and parameters; ctx.needs_input_grad turns into NULL pointers, an output nobody differentiated into a NULL upstream gradient."""
import torch

from . import ops, param_autograd

SLAB_ROWS = ops.AE_SLAB_ROWS      # rows per slab of the backward (bounds its scratch independently of n); tests use small values


def refuse_input_grad(**tensors):
    """points / feature rows / noise are not differentiable on this path."""
    param_autograd.refuse_input_grad("spec auto-encoder", **tensors)


def linear_params(ae):
    """The sixteen parameter tensors in ops.AE_PARAM_NAMES order."""
    lin = [ae.brdf_encoder_layer[2 * i] for i in range(5)] + [ae.brdf_decoder_layer[2 * i] for i in range(3)]
    return [t for l in lin for t in (l.weight, l.bias)]


class SparseAEFn(torch.autograd.Function):
    """Saves the points (or the feature rows), the noise, `var` and the parameters (param_autograd: what is saved, and why that way)."""

    @staticmethod
    def forward(ctx, ae, x, from_points, noise, *params):
        # autograd runs this with grad mode off: the module's forward_only_guard passes and the ordinary kernels run
        x = x.detach().float().contiguous()
        var = ae._var(x.device)
        enc = ae._encode_points(x) if from_points else ae._encode(x)
        act = ae._latent_act_code()
        sig_out = ae.out_act is not None
        if sig_out and getattr(ae.out_act, "__name__", "") != "sigmoid":
            raise NotImplementedError("out_act must be torch.sigmoid or None")
        dec = ae._blobs()[1]
        raw, _ = ops.ae_latent(enc, var, 2)
        if noise is None:
            lat, _ = ops.ae_latent(enc, var, act)
            out = ops.ae_decode(lat, dec, ae.out_dim, sig_out)
            out_xi = out.clone()
        else:
            noise = noise.detach().float().contiguous()
            lat, lat2 = ops.ae_latent(enc, var, act, noise, 0.01)
            out, out_xi = ops.ae_decode(lat, dec, ae.out_dim, sig_out), ops.ae_decode(lat2, dec, ae.out_dim, sig_out)
        ctx.present = (noise is not None, var is not None)
        ctx.save_for_backward(x, *([noise] if noise is not None else []), *([var] if var is not None else []), *params)
        ctx.cfg = (bool(from_points), act, sig_out, ae.in_dim, ae.out_dim, int(getattr(ae, "_train_slab_rows", 0) or SLAB_ROWS))
        ctx.set_materialize_grads(False)
        return out, out_xi, raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_out_xi, g_raw):
        saved = list(ctx.saved_tensors)
        x = saved.pop(0)
        noise = saved.pop(0) if ctx.present[0] else None
        var = saved.pop(0) if ctx.present[1] else None
        params = saved
        from_points, act, sig_out, in_dim, out_dim, slab = ctx.cfg
        X = ops.feat_pe10(x) if from_points else x
        want = tuple(k for k, need in zip(ops.AE_PARAM_NAMES, ctx.needs_input_grad[4:]) if need)
        if noise is None and g_out_xi is not None:           # out_xi was the clean output's copy
            g_out = g_out_xi if g_out is None else g_out + g_out_xi
            g_out_xi = None
        grads, _ = ops.ae_backward(X, params, g_out, g_out_xi, g_raw, noise=noise, var=var, latent_act=act, sigmoid_out=sig_out, in_dim=in_dim,
                                   out_dim=out_dim, want=want, slab_rows=slab)
        return param_autograd.backward_result(4, ops.AE_PARAM_NAMES, params, grads)


def _apply(ae, x, from_points, noise):
    if not ae.smooth_on_latent:
        raise NotImplementedError("SparseAE(smooth_on_latent=False): the HIP backward of the input-perturbed auto-encoders is not built")
    refuse_input_grad(points=x, noise=noise)
    return SparseAEFn.apply(ae, x, from_points, noise, *linear_params(ae))


def run_points(ae, pts, noise):
    """SparseAE.run_points with a graph to the auto-encoder's parameters: pts [n,3], noise [n,32] -> (out, out_xi, raw_latent)."""
    return _apply(ae, pts, True, noise)


def run_features(ae, X, noise=None):
    """The same from padded feature rows X [n,64] (SparseAE.run / SparseAE.encode's input after padding)."""
    return _apply(ae, X, False, noise)


class MaterialDecodeFn(torch.autograd.Function):
    """ops.material_decode (albedo = brdf[:3], roughness = brdf[3] 0.9 + 0.09, metallic = brdf[4] 0.99 + 0.01; the perturbed metallic is
    brdf_r[4] itself, model/sg_envmap_material.py:197-202) with its linear backward: six slices, plumbing."""

    @staticmethod
    def forward(ctx, brdf, brdf_r):
        ctx.set_materialize_grads(False)
        return ops.material_decode(brdf.detach(), brdf_r.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_alb, g_rough, g_metal, g_alb_r, g_rough_r, g_metal_r):
        def join(ga, gr, gm, rs, ms):
            if ga is None and gr is None and gm is None:
                return None
            ref = next(g for g in (ga, gr, gm) if g is not None)
            n = ref.shape[0]
            g = torch.zeros(n, 5, dtype=ref.dtype, device=ref.device)
            if ga is not None:
                g[:, :3] = ga
            if gr is not None:
                g[:, 3:4] = gr * rs
            if gm is not None:
                g[:, 4:5] = gm * ms
            return g
        return join(g_alb, g_rough, g_metal, 0.9, 0.99), join(g_alb_r, g_rough_r, g_metal_r, 0.9, 1.0)


def material_decode(brdf, brdf_r):
    return MaterialDecodeFn.apply(brdf, brdf_r)
