"""The stage losses under the reference's names, parameter order and defaults (model/loss.py): InvLoss (stages 3 and 4:
training/train_pbr.py:321, training/train_cesr.py:395), IllumLoss (the illumination stage) and query_indir_illum.  Only the interface is
the reference's -- names, parameters, attribute names, dict keys; every term is one of robir_amd.training's documented restatements.

InvLoss.forward's image term is the fused HIP op training.photometric_loss (tone map, masked distance, sum and gradient in one pass,
librobir_hip_photoloss.so).  hdr_fn: the bound hdr2ldr of an ACESToneMapping takes the fused path with that module's curve and shift (a
graph to adapt_illum if enable_tonemap_training marked it); any other callable is applied as given and followed by the fused masked distance
with the identity curve; None is the reference's x / (x + 1).  Tensors stay on the device of the model's outputs."""
import torch
from torch import nn

from . import nets, training

LOSS_TYPES = {"L1": nn.L1Loss, "L2": nn.MSELoss}


def _distance(loss_type, reduction):
    if loss_type not in LOSS_TYPES:
        raise Exception('Unknown loss_type!')
    return LOSS_TYPES[loss_type](reduction=reduction)


def _tone_of(hdr_fn):
    """The ACESToneMapping whose bound hdr2ldr `hdr_fn` is, else None."""
    owner = getattr(hdr_fn, "__self__", None)
    if isinstance(owner, nets.ACESToneMapping) and getattr(hdr_fn, "__func__", None) is nets.ACESToneMapping.hdr2ldr:
        return owner
    return None


class InvLoss(nn.Module):
    def __init__(self, idr_rgb_weight, eikonal_weight, mask_weight, alpha,
                 sg_rgb_weight, kl_weight, latent_smooth_weight,
                 brdf_multires=10, loss_type='L1'):
        super().__init__()
        given = dict(locals())
        for name in ("idr_rgb_weight", "eikonal_weight", "mask_weight", "alpha", "sg_rgb_weight", "kl_weight", "latent_smooth_weight",
                     "brdf_multires", "loss_type"):
            setattr(self, name, given[name])
        self.img_loss = _distance(loss_type, "sum")       # the attribute the reference holds; the fused op below does the work

    def _masked_distance(self, ldr, rgb_gt, network_object_mask, object_mask):
        from . import ops, tonemap_autograd
        return tonemap_autograd.image_loss(ldr, None, rgb_gt.to(ldr.device), network_object_mask, object_mask, None, ops.PL_CURVE_IDENTITY,
                                           l2=self.loss_type == "L2")

    def get_rgb_loss(self, rgb_values, rgb_gt, network_object_mask, object_mask):
        """model/loss.py:31-42 on already tone-mapped values: the summed L1 / L2 distance over the rows inside both masks, divided by the
        number of all rows -- the fused masked distance with the identity curve (0 for an empty mask)."""
        return self._masked_distance(rgb_values, rgb_gt, network_object_mask, object_mask)

    def get_eikonal_loss(self, grad_theta):
        return training.eikonal_loss(grad_theta)

    def get_mask_loss(self, sdf_output, network_object_mask, object_mask):
        return training.mask_loss(sdf_output, network_object_mask, object_mask, self.alpha)

    def get_latent_smooth_loss(self, model_outputs):
        return training.latent_smooth(model_outputs)

    def get_normal_loss(self, model_outputs):
        return training.normal_loss(model_outputs["normal_map"], model_outputs["normals"], model_outputs["surface_mask"])

    def kl_divergence(self, rho, rho_hat):
        return training.kl_sparsity(rho_hat, rho)

    def get_kl_loss(self, model, points, train_spec):
        """model/loss.py:81-95: the KL sparsity (rho = 0.05) of the pre-activation latent that the auto-encoder `train_spec` selects gives the
        embedded points.  The embedding is the model's brdf_embed_fn where it has one, else the brdf_multires-band embedder."""
        embed = getattr(model, "brdf_embed_fn", None)
        if embed is None:
            from . import embedder
            embed = embedder.get_embedder(self.brdf_multires)[0]
        layer = model.spec_brdf_encoder_layer if train_spec else model.brdf_encoder_layer
        return self.kl_divergence(0.05, layer.encode(embed(points)))

    def forward(self, model_outputs, ground_truth, mat_model=None, train_idr=False, train_spec=False, hdr_fn=None):
        out = model_outputs
        hit, inside = out["network_object_mask"], out["object_mask"]
        target = ground_truth["rgb"].to(out["sg_rgb"].device)
        tone = _tone_of(hdr_fn)
        if hdr_fn is None or tone is not None:       # tone map, distance, sum and gradient in one pass
            image = training.photometric_loss(out["sg_rgb"], out["indir_rgb"], target, hit, inside, tone=tone, loss_type=self.loss_type)
        else:
            image = self._masked_distance(hdr_fn(out["sg_rgb"] + out["indir_rgb"]), target, hit, inside)
        terms = {"sg_rgb_loss": image,
                 "kl_loss": self.get_kl_loss(mat_model, out["points"][hit], train_spec) * self.kl_weight,
                 "latent_smooth_loss": self.get_latent_smooth_loss(out) * self.latent_smooth_weight,
                 "normal_loss": self.get_normal_loss(out)}
        terms["loss"] = image * self.sg_rgb_weight          # the reference's total holds the image term alone (loss.py:116)
        return terms


def query_indir_illum(lgtSGs, sample_dirs):
    return training.query_indir_illum(lgtSGs, sample_dirs)


class IllumLoss(nn.Module):
    def __init__(self, loss_type='L1'):
        super().__init__()
        self.loss_type = loss_type
        self.rgb_loss = _distance(loss_type, "mean")

    def forward(self, model_outputs, trace_outputs, anneal_t):
        """model/loss.py:156-179 -> (radiance term, visibility term)."""
        radiance = training.radiance_loss(model_outputs, trace_outputs, anneal_t, loss_type=self.loss_type)
        visibility = training.visibility_loss(trace_outputs["pred_vis"], trace_outputs["gt_vis"], model_outputs["network_object_mask"])
        return radiance, visibility
