"""Opt-in training of the material network's spec auto-encoder on the HIP path (stage 3 of the reference, training/train_pbr.py:104-105,
348-396: the optimiser holds spec_brdf_encoder_layer, lgtSGs and specular_reflectance).

Nothing here is on by default: every network stays forward-only behind nets.forward_only_guard until enable_material_training marks an
EnvmapMaterialNetwork.  With the mark, grad mode on and a parameter that requires grad,

  * EnvmapMaterialNetwork.forward(points, train_spec=True) returns sg_diffuse_albedo / sg_roughness / sg_metallic and the three random_xi_*
    material outputs with a graph to the spec auto-encoder's parameters (robir_amd/ae_autograd.py -> librobir_hip_train.so); sg_lgtSGs and
    sg_specular_reflectance are the parameters themselves; the normal-map outputs carry no graph (no stage-3 loss term reaches them);
  * SparseAE.encode of the marked auto-encoder is differentiable (the KL term's input);
  * train_spec=False detaches the material outputs like the reference does.

kl_sparsity / latent_smooth restate the two stage-3 regularisers of model/loss.py:61-95 on tensors (a few reductions: plumbing).

The same opt-in exists for the "Vis" stage (training/train_visibility.py:297-308: the optimiser holds visibility_network):
enable_visibility_training marks a VisNetwork.  With the mark, grad mode on and a parameter that requires grad, VisNetwork.forward /
logits_from_points return logits with a graph to the ten nn.Linear tensors (robir_amd/vis_autograd.py -> librobir_hip_vistrain.so), and
IDRNetwork.trace_radiance's pred_vis carries that graph; visibility_loss restates the stage's cross-entropy (model/loss.py:173-177).

The stage's other optimiser step (training/train_visibility.py:309-313) trains indirect_illum_network: enable_illumination_training marks an
IndirctIllumNetwork.  With the mark, grad mode on and a parameter that requires grad, IndirctIllumNetwork.forward returns (lgt_sgs, env_int)
with a graph to lobe_layer and integral_layer (robir_amd/illum_autograd.py -> librobir_hip_illumtrain.so, librobir_hip_train.so), the model's
indirect_sgs / indir_integral carry it, and radiance_loss restates model/loss.py:156-171 on the fused, differentiable query_indir_illum.

The CESR stage (training/train_cesr.py:107-117: the optimiser holds shadow_net and normal_net): enable_cesr_training marks an SDFNetwork of
kind shadow or normal.  With the mark, grad mode on and a parameter that requires grad, SDFNetwork.forward / eval_point_labels / diffuse_vis /
unit_normal return outputs with a graph to the 27 weight-norm tensors (robir_amd/cesr_autograd.py -> librobir_hip_cesrtrain.so), and
renderer.CESRHook carries it into the shading (diffuse_vis) and into the normal-consistency term of gradient_error (normal_new).

The image loss that drives all of them (model/loss.py:97-125, called by training/train_pbr.py:321 and train_cesr.py:395):
enable_tonemap_training marks an ACESToneMapping.  With the mark and grad mode on, hdr2ldr / ldr2hdr return the same bits plus a graph to x,
to a raw_shift tensor and -- raw_shift=None -- to adapt_illum (robir_amd/tonemap_autograd.py -> librobir_hip_photoloss.so);
photometric_loss is the fused tone map + masked L1 / L2 + gradient, white_loss the runner's light prior; eikonal_loss, mask_loss and
normal_loss restate the remaining terms of model/loss.py:44-73; robir_amd/loss.py assembles InvLoss / IllumLoss from these pieces."""
import torch

from . import nets


def _material_network(obj):
    if isinstance(obj, nets.EnvmapMaterialNetwork):
        return obj
    net = getattr(obj, "envmap_material_network", None)
    if isinstance(net, nets.EnvmapMaterialNetwork):
        return net
    return None


def enable_material_training(net, on=True):
    """Mark (on=False: unmark) an EnvmapMaterialNetwork -- or the one a model holds as .envmap_material_network -- and its
    spec_brdf_encoder_layer as trainable on the HIP path.  Returns the material network.  A SparseAE may be passed directly; one with
    smooth_on_latent=False (the normal decoder, the indirect-illumination integral layer) is refused: its backward is not built."""
    if isinstance(net, nets.SparseAE):
        if on and not net.smooth_on_latent:
            raise NotImplementedError("enable_material_training: the backward of an input-perturbed auto-encoder (smooth_on_latent=False: the "
                                      "normal decoder, the indirect-illumination integral layer) is not built -- only the latent-smoothed "
                                      "spec auto-encoder trains on the HIP path")
        net._material_training = bool(on)
        return net
    mat = _material_network(net)
    if mat is None:
        raise TypeError(f"enable_material_training: {type(net).__name__} is neither an EnvmapMaterialNetwork nor a model that has one")
    enable_material_training(mat.spec_brdf_encoder_layer, on)
    mat._material_training = bool(on)
    return mat


def material_training_enabled(net):
    mat = net if isinstance(net, nets.SparseAE) else _material_network(net)
    return bool(getattr(mat, "_material_training", False))


def kl_sparsity(raw_latent, rho=0.05):
    """The KL sparsity term on a pre-activation latent [n,32] (model/loss.py:75-79 with SparseAE.kl_divergence,
    model/sg_envmap_material.py:101-105): rho_hat = mean over the rows of sigmoid(latent);
    mean_j( rho log(rho / (rho_hat_j + 1e-4)) + (1 - rho) log((1 - rho) / (1 - rho_hat_j + 1e-4)) )."""
    rho_hat = torch.mean(torch.sigmoid(raw_latent.reshape(-1, raw_latent.shape[-1])), 0)
    rho = torch.full_like(rho_hat, float(rho))
    return torch.mean(rho * torch.log(rho / (rho_hat + 1e-4)) + (1 - rho) * torch.log((1 - rho) / (1 - rho_hat + 1e-4)))


def latent_smooth(out):
    """The latent-smoothness term (model/loss.py:61-67): L1(albedo, random_xi albedo) + 0.2 L1(roughness, random_xi roughness), each a mean.
    `out`: a dict with the model's keys (diffuse_albedo, roughness) or the material network's (sg_diffuse_albedo, sg_roughness), next to
    random_xi_diffuse_albedo / random_xi_roughness."""
    pick = lambda k: out[k] if k in out else out["sg_" + k]
    d_diff, d_rough = pick("diffuse_albedo"), pick("roughness")[..., 0]
    d_xi_diff, d_xi_rough = out["random_xi_diffuse_albedo"], out["random_xi_roughness"][..., 0]
    return torch.mean(torch.abs(d_diff - d_xi_diff)) + torch.mean(torch.abs(d_rough - d_xi_rough)) * 0.2


def _visibility_network(obj):
    if isinstance(obj, nets.VisNetwork):
        return obj
    net = getattr(obj, "visibility_network", None)
    if isinstance(net, nets.VisNetwork):
        return net
    return None


def enable_visibility_training(net, on=True):
    """Mark (on=False: unmark) a VisNetwork -- or the one a model holds as .visibility_network -- as trainable on the HIP path.  Returns the
    visibility network.  The fused consumers of its weights (the light-visibility kernel, the BRDF-lobe visibilities, the CESR hook) stay
    non-differentiable; they read parameter-version-keyed blobs and see an optimiser step on their next call."""
    vis = _visibility_network(net)
    if vis is None:
        raise TypeError(f"enable_visibility_training: {type(net).__name__} is neither a VisNetwork nor a model that has one")
    vis._visibility_training = bool(on)
    return vis


def visibility_training_enabled(net):
    return bool(getattr(_visibility_network(net), "_visibility_training", False))


def visibility_loss(pred_vis, gt_vis, points_mask):
    """The visibility term of IllumLoss.forward (model/loss.py:173-177): nn.CrossEntropyLoss() (mean over the rows) of the logits
    pred_vis [N,S,2] at the surface points points_mask [N]; the class index is the NEGATED traced label gt_vis [N,S,1] (bool: the secondary
    ray hit the surface), so class 1 = visible."""
    mask = points_mask.reshape(-1).bool()
    pred = pred_vis[mask].reshape(-1, 2)
    gt = (~gt_vis[mask].bool()).long().reshape(-1)
    return torch.nn.functional.cross_entropy(pred, gt)


def enable_cesr_training(net, on=True):
    """Mark (on=False: unmark) an SDFNetwork of kind shadow or normal -- the CESR stage's shadow_net / normal_net -- as trainable on the HIP
    path.  Returns the network.  The NeuS-shape SDFNetwork is refused: its backward is not built."""
    if not isinstance(net, nets.SDFNetwork):
        raise TypeError(f"enable_cesr_training: {type(net).__name__} is not an SDFNetwork")
    if net.kind == "neus":
        raise NotImplementedError("enable_cesr_training: the backward of the NeuS-shape SDFNetwork (3 -> 257, 256 x 8) is not built -- only "
                                  "the CESR stage's shadow_net (191 -> 2) and normal_net (63 -> 3) train on the HIP path")
    net._cesr_training = bool(on)
    return net


def cesr_training_enabled(net):
    return isinstance(net, nets.SDFNetwork) and bool(getattr(net, "_cesr_training", False))


def _illumination_network(obj):
    if isinstance(obj, nets.IndirctIllumNetwork):
        return obj
    net = getattr(obj, "indirect_illum_network", None)
    if isinstance(net, nets.IndirctIllumNetwork):
        return net
    return None


def enable_illumination_training(net, on=True):
    """Mark (on=False: unmark) an IndirctIllumNetwork -- or the one a model holds as .indirect_illum_network -- as trainable on the HIP path.
    Returns the illumination network.  Its integral_layer stays unmarked: the network's forward differentiates it as one clean pass on the
    perturbed rows, the stand-alone SparseAE(smooth_on_latent=False) forward keeps its refusal."""
    ill = _illumination_network(net)
    if ill is None:
        raise TypeError(f"enable_illumination_training: {type(net).__name__} is neither an IndirctIllumNetwork nor a model that has one")
    ill._illumination_training = bool(on)
    return ill


def illumination_training_enabled(net):
    return bool(getattr(_illumination_network(net), "_illumination_training", False))


def query_indir_illum(lgtSGs, sample_dirs):
    """model/loss.py:128-141 under the reference's name and argument order, fused and differentiable in the lobes: lgtSGs [n,L,7],
    sample_dirs [n,S,3] -> radiance [n,S,3] = sum_j mu_j exp(lambda_j (d . l_j / |l_j| - 1)).  sample_dirs is a constant."""
    from . import illum_autograd
    return illum_autograd.sg_query(lgtSGs, sample_dirs)


def radiance_loss(model_outputs, trace_outputs, anneal_t=0.0, loss_type="L1", query=None):
    """The radiance term of IllumLoss.forward (model/loss.py:156-171): with points_mask = network_object_mask [N] and indir_mask [N,S], the
    mean L1 (loss_type "L2": mean squared) distance between trace_radiance[indir_mask] + anneal_t and
    query(indirect_sgs[points_mask], sample_dirs)[indir_mask[points_mask]], plus the same distance between gt_integral[points_mask] and
    indir_integral[points_mask].  query: query_indir_illum's signature; the fused one by default."""
    if loss_type == "L1":
        dist = torch.nn.functional.l1_loss
    elif loss_type == "L2":
        dist = torch.nn.functional.mse_loss
    else:
        raise ValueError(f"radiance_loss: unknown loss_type {loss_type!r} (L1 | L2)")
    query = query or query_indir_illum
    indir_mask = trace_outputs["indir_mask"].bool()
    points_mask = model_outputs["network_object_mask"].reshape(-1).bool()
    gt_radiance = trace_outputs["trace_radiance"][indir_mask] + anneal_t
    pred_radiance = query(model_outputs["indirect_sgs"][points_mask], trace_outputs["sample_dirs"])
    loss = dist(pred_radiance[indir_mask[points_mask]], gt_radiance)
    return loss + dist(model_outputs["indir_integral"][points_mask], trace_outputs["gt_integral"][points_mask])


def _tone_mapper(obj):
    if isinstance(obj, nets.ACESToneMapping):
        return obj
    if isinstance(obj, nets.GammaCorrect):
        return obj.hdr_shift
    gamma = getattr(obj, "gamma", None)
    if isinstance(gamma, nets.GammaCorrect):
        return gamma.hdr_shift
    return None


def enable_tonemap_training(obj, on=True):
    """Mark (on=False: unmark) an ACESToneMapping -- or the one a GammaCorrect holds as .hdr_shift, or the one of a model's .gamma -- as
    differentiable on the HIP path.  Returns the tone mapper.  With the mark and grad mode on, hdr2ldr / ldr2hdr return today's bits plus a
    graph to x, to a raw_shift tensor and, for raw_shift=None, to adapt_illum (robir_amd/tonemap_autograd.py -> librobir_hip_photoloss.so);
    a deferred x, no_grad and an unmarked module behave as before."""
    tone = _tone_mapper(obj)
    if tone is None:
        raise TypeError(f"enable_tonemap_training: {type(obj).__name__} is neither an ACESToneMapping, a GammaCorrect nor a model that has .gamma")
    tone._tonemap_training = bool(on)
    return tone


def tonemap_training_enabled(obj):
    return bool(getattr(_tone_mapper(obj), "_tonemap_training", False))


def photometric_loss(sg_rgb, indir_rgb, rgb_gt, network_object_mask, object_mask, tone=None, raw_shift=None, loss_type="L1"):
    """The image term of InvLoss.forward (model/loss.py:31-42,97-110) as ONE fused, differentiable op: with m = network_object_mask &
    object_mask [N] and pred = tone.hdr2ldr(sg_rgb + indir_rgb, raw_shift), sum_m sum_c |pred - rgb_gt| (loss_type "L2": squared) / N, N all
    rows.  indir_rgb may be None.  tone: an ACESToneMapping (or what enable_tonemap_training accepts); None gives the reference's fallback
    pred = x / (x + 1).  Gradients reach sg_rgb and indir_rgb, and -- only for a tone marked by enable_tonemap_training -- a raw_shift
    tensor or, for raw_shift=None, adapt_illum through as_input(); an unmarked tone is a constant curve."""
    from . import ops, tonemap_autograd
    if loss_type not in ("L1", "L2"):
        raise ValueError(f"photometric_loss: unknown loss_type {loss_type!r} (L1 | L2)")
    shift, curve = None, ops.PL_CURVE_RATIONAL
    if tone is not None:
        tm = _tone_mapper(tone)
        if tm is None:
            raise TypeError(f"photometric_loss: tone is a {type(tone).__name__}, not an ACESToneMapping")
        curve = tm._curve
        if curve != ops.PL_CURVE_IDENTITY:
            marked = tonemap_training_enabled(tm) and torch.is_grad_enabled()
            shift = tm.as_input() if raw_shift is None else raw_shift
            if not isinstance(shift, torch.Tensor):
                shift = torch.tensor(float(shift), device=sg_rgb.device)
            shift = shift.to(sg_rgb.device).float()
            if not marked:
                shift = shift.detach()
    return tonemap_autograd.image_loss(sg_rgb, indir_rgb, rgb_gt.to(sg_rgb.device), network_object_mask, object_mask, shift, curve,
                                       l2=loss_type == "L2")


def white_loss(lgtSGs):
    """The white-light prior of the stage-3 runner (training/train_pbr.py:313-316) on tensors: 0.01 times the mean over the lobes of the
    variance of |mu| / (|mu|_2 + 1e-4) across the three channels."""
    lgt = torch.abs(lgtSGs[..., -3:])
    mu = lgt.norm(dim=-1, keepdim=True) + 1e-4
    return (lgt / mu).var(-1).mean() * 0.01


def eikonal_loss(grad_theta):
    """The eikonal term (model/loss.py:44-49): mean over the rows of (|grad_theta|_2 - 1)^2 for SDF gradients [n,3]; 0 for n = 0."""
    if grad_theta.shape[0] == 0:
        return torch.zeros((), dtype=torch.float32, device=grad_theta.device)
    length = torch.linalg.vector_norm(grad_theta, ord=2, dim=1)
    return torch.mean(torch.square(length - 1.0))


def mask_loss(sdf_output, network_object_mask, object_mask, alpha):
    """The silhouette term (model/loss.py:51-59).  Over the rows OUTSIDE network_object_mask & object_mask, the summed binary cross entropy
    between the logits -alpha * sdf and the target object_mask, divided by alpha and by the number N of all rows; 0 if there is no such row."""
    outside = torch.logical_not(torch.logical_and(network_object_mask, object_mask))
    if not bool(outside.any()):
        return torch.zeros((), dtype=torch.float32, device=sdf_output.device)
    logits = (sdf_output[outside] * (-alpha)).squeeze()
    target = object_mask[outside].to(logits.dtype)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, target, reduction="sum")
    return bce / (alpha * float(object_mask.shape[0]))


def normal_loss(normal_map, normals, surface_mask):
    """The normal term (model/loss.py:69-73): the mean squared difference between the predicted normal map and the geometry's normals over
    the rows of surface_mask."""
    keep = surface_mask.reshape(-1).bool()
    return torch.nn.functional.mse_loss(normal_map.reshape(-1, normal_map.shape[-1])[keep], normals.reshape(-1, normals.shape[-1])[keep])
