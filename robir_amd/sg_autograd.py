"""Differentiable SG shading: a torch.autograd.Function around the kernel pair rb_sg_shade / rb_sg_shade_bwd.

Differentiable inputs: the light SGs ([M,7] shared -> gradient [M,7] summed over the points on the device; [n,M,7] per point), the scalar
specular reflectance f0 (any shape with one element), roughness, albedo, metallic, the indirect integral -- and, at this level, the two
visibilities bvis [n] / light_vis [n,M], which enter the shaded colour linearly.  normal and view are constants: geometry is out of scope
of the backward and a tensor that requires grad there raises NotImplementedError instead of receiving a silent zero.  The forward saves its
inputs and the two clamped outputs; the backward is ONE rb_sg_shade_bwd call that recomputes everything per (point, lobe) and allocates only
the gradients that were asked for (ctx.needs_input_grad -> NULL pointers), so no [n,M] tensor exists unless d light_vis is wanted."""
import torch

from . import ops

_NAMES = ("lgt", "f0", "rough", "albedo", "bvis", "light_vis", "metallic", "indir_integral")


def refuse_geometry_grad(**tensors):
    """points / normal / viewdirs are not differentiable on this path: say so instead of returning a zero gradient."""
    if not torch.is_grad_enabled():
        return
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError(f"robir_amd SG shading has no gradient with respect to `{name}` (geometry is frozen in the HIP backward: "
                                      f"pass {name}.detach(), or differentiate geometry on the reference's modules)")


def wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def shared_light(lgtSGs):
    """[M,7] tensor standing for a light that every point shares -- lgtSGs itself when 2-D, else the tensor an expanded view
    (stride(0) == 0, what render_with_all_sg callers pass) was expanded from, found through Tensor._base -- so that its gradient arrives as
    [M,7] summed on the device and not as an [n,M,7] tensor.  That holds when the view's base is a contiguous tensor of exactly M x 7 elements
    (`p.unsqueeze(0).expand(n, M, 7)`, with or without a non-view op before it); any other expanded view falls back to lgtSGs[0], see below.
    None when lgtSGs is a genuine per-point light."""
    if lgtSGs.dim() == 2:
        return lgtSGs
    if lgtSGs.stride(0) != 0:
        return None
    M = lgtSGs.shape[1]
    base = lgtSGs._base
    if (base is not None and base.numel() == M * 7 and base.is_contiguous() and base.storage_offset() == lgtSGs.storage_offset()
            and tuple(lgtSGs.stride()[1:]) == (7, 1)):
        return base.reshape(M, 7)
    # an expanded view of something that is not a plain contiguous [M,7] tensor (a slice of a larger parameter, ...): still correct, but
    # autograd's select-backward then routes this gradient through an [n,M,7] zeros tensor (INTEGRATION 6a states the caveat)
    return lgtSGs[0]


_SAVED = ("normal", "view", "lgt", "f0", "rough", "albedo", "bvis", "light_vis", "metallic", "indir_integral")


class SgShadeFn(torch.autograd.Function):
    """Every tensor the backward needs -- the detached fp32 inputs and the two clamped outputs -- goes through ctx.save_for_backward: the
    outputs must not sit on ctx as plain attributes (output -> grad_fn -> ctx -> output is a reference cycle only the cyclic collector frees,
    and the sampled light_vis [n,M] would stay allocated with it), autograd checks the inputs for in-place changes, and everything is released
    with the graph.  ctx keeps only non-tensor items."""

    @staticmethod
    def forward(ctx, normal, view, lgt, f0, rough, albedo, bvis, light_vis, metallic, indir_integral, lin_diff):
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        a = dict(normal=f32(normal), view=f32(view), lgt=f32(lgt), f0=f32(f0).reshape(-1)[:1], rough=f32(rough).reshape(-1), albedo=f32(albedo),
                 bvis=f32(bvis).reshape(-1), light_vis=f32(light_vis), metallic=None if metallic is None else f32(metallic).reshape(-1),
                 indir_integral=f32(indir_integral))
        rgb, spec, diff, shadow = ops.sg_shade(a["normal"], a["view"], a["lgt"], a["f0"], a["rough"], a["albedo"], a["bvis"],
                                               light_vis=a["light_vis"], metallic=a["metallic"], indir_integral=a["indir_integral"],
                                               lin_diff=lin_diff, want_shadow=True)
        ctx.present = tuple(k for k in _SAVED if a[k] is not None)
        ctx.save_for_backward(*(a[k] for k in ctx.present), spec, diff)
        ctx.lin_diff = bool(lin_diff)
        ctx.shapes = {k: (None if t is None else (t.shape, t.dtype)) for k, t in
                      dict(lgt=lgt, f0=f0, rough=rough, albedo=albedo, bvis=bvis, light_vis=light_vis, metallic=metallic,
                           indir_integral=indir_integral).items()}
        ctx.mark_non_differentiable(shadow)
        return rgb, spec, diff, shadow

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_spec, g_diff, g_shadow):
        saved = ctx.saved_tensors
        a = dict.fromkeys(_SAVED)
        a.update(zip(ctx.present, saved))
        spec, diff = saved[-2], saved[-1]
        z = lambda g: torch.zeros_like(spec) if g is None else g.float()
        g_rgb = z(g_rgb)
        gs, gd = (z(g_spec) + g_rgb).contiguous(), (z(g_diff) + g_rgb).contiguous()
        needs = dict(zip(_NAMES, ctx.needs_input_grad[2:10]))
        want = tuple(k for k in _NAMES if needs[k] and a[k] is not None)
        out = ops.sg_shade_backward(a["normal"], a["view"], a["lgt"], a["f0"], a["rough"], a["albedo"], a["bvis"], spec, diff, gs, gd,
                                    light_vis=a["light_vis"], metallic=a["metallic"], indir_integral=a["indir_integral"], lin_diff=ctx.lin_diff,
                                    want=want)
        grads = []
        for k in _NAMES:
            if k not in out:
                grads.append(None)
                continue
            shape, dtype = ctx.shapes[k]
            g = out[k]
            if k == "f0" and g.numel() != shape.numel():        # only the first element is read by the forward
                full = torch.zeros(shape.numel(), dtype=g.dtype, device=g.device)
                full[:1] = g
                g = full
            grads.append(g.reshape(shape).to(dtype))
        return (None, None, *grads, None)


def sg_shade(normal, view, lgt, f0, rough, albedo, bvis, light_vis=None, metallic=None, indir_integral=None, lin_diff=False):
    """ops.sg_shade with autograd: -> (rgb, spec, diff, shadow), each [n,3]; shadow carries no gradient.  lgt [M,7] or [n,M,7]."""
    refuse_geometry_grad(normal=normal, viewdirs=view)
    if not isinstance(f0, torch.Tensor):
        f0 = torch.full((1,), float(f0), device=normal.device)
    return SgShadeFn.apply(normal, view, lgt, f0, rough, albedo, bvis, light_vis, metallic, indir_integral, bool(lin_diff))
