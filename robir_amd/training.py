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
IDRNetwork.trace_radiance's pred_vis carries that graph; visibility_loss restates the stage's cross-entropy (model/loss.py:173-177)."""
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
