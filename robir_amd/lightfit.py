"""Light SGs of a user's environment map: what the reference's envmaps/fit_envmap_with_sg.py does with PyTorch autograd, on the device
(librobir_hip_lightfit.so, include/robir_hip_lightfit.h).

  render_envmap_sg / compute_envmap   the reference's signatures (model/sg_render.py:9-42), differentiable in lgtSGs: the forward is the
                                      existing rb_envmap_sg (ops.envmap_sg), the backward rb_lf_envmap_sg_bwd.  With grad mode off, or
                                      nothing requiring grad, exactly sg_render's forward-only result.  sg_render's own two functions keep
                                      detaching; other objectives than the MSE use these with any torch optimiser.
  area_resize                         the exact area-weighted down-sample (cv2.INTER_AREA when shrinking).
  fit_envmap                          the fit: forward, MSE, gradient and torch.optim.Adam's update fused into rb_lf_fit_steps, enqueued in
                                      blocks without a host round trip.

`python -m robir_amd.fit_light` is the command line around fit_envmap."""
import ctypes

import numpy as np
import torch

from . import _lib, ops, param_autograd
from ._lib import c_int, c_long, ptr, stream_ptr

c_double = ctypes.c_double


def _scratch(n, M, dev):
    need = _lib.lightfit().rb_lf_scratch_bytes(c_long(n), c_int(M))
    if need < 0:
        raise _lib.RobirHipError("rb_lf_scratch_bytes: " + _lib.aux_error(_lib.lightfit()))
    return torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev), need


def envmap_sg_backward(lgt, dirs, g_rgb):
    """d <g_rgb, render_envmap_sg(lgt, dirs)> / d lgt: lgt [M,7], dirs [n,3], g_rgb [n,3] fp32 device tensors -> [M,7] fp32."""
    lgt, dirs, g_rgb = ops._f32(lgt), ops._f32(dirs), ops._f32(g_rgb)
    M, n = lgt.shape[0], dirs.shape[0]
    d_lgt = torch.zeros(M, 7, dtype=torch.float32, device=lgt.device)
    if n:
        scratch, nbytes = _scratch(n, M, lgt.device)
        _lib.call_lightfit("rb_lf_envmap_sg_bwd", ptr(lgt), c_int(M), ptr(dirs), c_long(n), ptr(g_rgb), ptr(d_lgt), ptr(scratch), c_long(nbytes),
                           stream_ptr())
    return d_lgt


class EnvmapSgFn(torch.autograd.Function):
    """rgb [n,3] of (lgt [M,7], dirs [n,3]); differentiable in lgt.  Saves its two inputs, nothing else (param_autograd)."""

    @staticmethod
    def forward(ctx, lgt, dirs):
        ctx.save_for_backward(lgt, dirs)
        ctx.set_materialize_grads(False)
        return ops.envmap_sg(lgt, dirs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lgt, dirs = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        return envmap_sg_backward(lgt, dirs, g.float().contiguous()), None


def render_envmap_sg(lgtSGs, viewdirs):
    """sum_k mu_k exp(lambda_k (d.lobe_k - 1)) (sg_render.py:26-42), differentiable in lgtSGs."""
    param_autograd.refuse_input_grad("light-SG environment map", viewdirs=viewdirs)
    shape = list(viewdirs.shape[:-1]) + [3]
    d = viewdirs.detach().to(lgtSGs.device).reshape(-1, 3).float().contiguous()
    if torch.is_grad_enabled() and lgtSGs.requires_grad:
        return EnvmapSgFn.apply(lgtSGs.float().contiguous(), d).reshape(shape)
    return ops.envmap_sg(lgtSGs.detach().float().contiguous(), d).reshape(shape)


def envmap_dirs(H, W, upper_hemi=False):
    """The direction grid of compute_envmap (sg_render.py:9-23), [H, W, 3] fp32 on the CPU."""
    phi, theta = torch.meshgrid([torch.linspace(0.0, np.pi / 2.0 if upper_hemi else np.pi, H),
                                 torch.linspace(1.0 * np.pi, -1.0 * np.pi, W)], indexing="ij")
    return torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], -1)


def compute_envmap(lgtSGs, H, W, upper_hemi=False):
    return render_envmap_sg(lgtSGs, envmap_dirs(H, W, upper_hemi)).reshape(H, W, 3)


def _device_rgb(img, dev=None):
    """[H0, W0, >= 3] torch tensor or numpy array -> contiguous fp32 [H0, W0, 3] on the device."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(img)[:, :, :3], dtype=np.float32))
    if t.dim() != 3 or t.shape[2] < 3:
        raise ValueError(f"an image [H, W, >= 3] is needed, got {tuple(t.shape)}")
    if dev is None:
        dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.detach()[:, :, :3].to(dev).float().contiguous()


def area_resize(img, H, W):
    """Exact area-weighted down-sample of img [H0, W0, >= 3] to [H, W, 3] (fp32, on the device): every destination pixel is the
    coverage-weighted mean of the source pixels under its footprint.  Up-sampling is refused."""
    src = _device_rgb(img)
    dst = torch.empty(int(H), int(W), 3, dtype=torch.float32, device=src.device)
    _lib.call_lightfit("rb_lf_area_resize", ptr(src), c_int(src.shape[0]), c_int(src.shape[1]), ptr(dst), c_int(int(H)), c_int(int(W)), stream_ptr())
    return dst


def init_light_sgs(num_sg, seed=0):
    """The reference's initialisation (fit_envmap_with_sg.py:37-38): randn(M, 7) with the sharpness column x 100, from a CPU generator."""
    sg = torch.randn(num_sg, 7, generator=torch.Generator().manual_seed(int(seed)))
    sg[:, 3:4] *= 100.0
    return sg


def fit_envmap(envmap, num_sg=128, iters=100000, lr=1e-2, size=(256, 512), init=None, seed=0, block=1000, callback=None, state=None,
               betas=(0.9, 0.999), eps=1e-8):
    """Fit num_sg light SGs to envmap [H0, W0, >= 3] (torch tensor or numpy array) like the reference's fit_envmap_with_sg.py: the map is
    area-resized to `size` (never up-sampled: an axis shorter than the target keeps its length), the loss is the plain mean squared error on
    compute_envmap's direction grid, the optimiser is torch.optim.Adam(lr) -- all of it inside rb_lf_fit_steps, `block` steps per call.

    init      [num_sg, 7] to start from (a saved sg_*.npy) in place of the reference's random initialisation from `seed`
    callback  called after every block as callback(step, loss, lgtSGs): steps done so far, the block's last loss, the current parameters
              (the device tensor the fit goes on updating: copy what is to be kept).  Reading a block's losses is the only synchronisation.
    state     a dict.  On entry 'adam_m', 'adam_v' [num_sg, 7] and 'step' continue an earlier fit (absent: zero moments, step 0, which is
              the reference's resume); after every block, before the callback, it holds the current three.

    -> (lgtSGs [num_sg, 7] fp32 on the device, the loss before each of the `iters` updates as a float64 numpy array).
    A loss that is not finite raises FloatingPointError naming the step; its `lgtSGs` / `step` attributes are the state at the start of the
    block in which it happened, and the callback is not called for that block."""
    src = _device_rgb(envmap)
    dev = src.device
    H, W = min(int(size[0]), src.shape[0]), min(int(size[1]), src.shape[1])
    target = area_resize(src, H, W).reshape(-1, 3)
    dirs = envmap_dirs(H, W).reshape(-1, 3).to(dev).contiguous()
    n = H * W
    if init is None:
        lgt = init_light_sgs(num_sg, seed)
    else:
        lgt = torch.as_tensor(np.asarray(init) if not isinstance(init, torch.Tensor) else init).detach().float()
        if tuple(lgt.shape) != (num_sg, 7):
            raise ValueError(f"init has shape {tuple(lgt.shape)}, not ({num_sg}, 7)")
    lgt = lgt.to(dev).clone().contiguous()
    state = {} if state is None else state
    moment = lambda k: (torch.as_tensor(state[k]).detach().float().to(dev).clone().contiguous() if state.get(k) is not None
                        else torch.zeros(num_sg, 7, dtype=torch.float32, device=dev))
    adam_m, adam_v, step = moment("adam_m"), moment("adam_v"), int(state.get("step") or 0)
    if tuple(adam_m.shape) != (num_sg, 7) or tuple(adam_v.shape) != (num_sg, 7):
        raise ValueError(f"state moments must have shape ({num_sg}, 7)")
    state.update(adam_m=adam_m, adam_v=adam_v, step=step)
    scratch, nbytes = _scratch(n, num_sg, dev)
    iters, block = int(iters), max(1, int(block))
    hist = np.zeros(iters, dtype=np.float64)
    done = 0
    while done < iters:
        k = min(block, iters - done)
        start = (lgt.clone(), step)
        losses = torch.empty(k, dtype=torch.float64, device=dev)
        _lib.call_lightfit("rb_lf_fit_steps", ptr(lgt), ptr(adam_m), ptr(adam_v), c_int(num_sg), ptr(dirs), ptr(target), c_long(n), c_long(step),
                           c_long(k), c_double(lr), c_double(betas[0]), c_double(betas[1]), c_double(eps), ptr(losses), ptr(scratch),
                           c_long(nbytes), stream_ptr())
        block_losses = losses.cpu().numpy()
        bad = np.flatnonzero(~np.isfinite(block_losses))
        if bad.size:
            err = FloatingPointError(f"the loss is not finite ({block_losses[bad[0]]}) at step {step + int(bad[0])}: the fit stopped; "
                                     f"the parameters at step {start[1]} are in this error's `lgtSGs`")
            err.lgtSGs, err.step = start
            raise err
        hist[done:done + k] = block_losses
        done += k
        step += k
        state.update(adam_m=adam_m, adam_v=adam_v, step=step)
        if callback is not None:
            callback(step, float(block_losses[-1]), lgt)
    return lgt, hist
