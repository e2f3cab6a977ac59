"""Drop-in for model/implicit_differentiable_renderer.py:261-650 (IDRNetwork) on the HIP kernels, plus the
MI355X-first batched renderer that bench.py times.

IDRNetwork(conf): same sub-module names / state-dict keys / methods the stage runners reach for:
  .implicit_network .ray_tracer .octree_ray_tracer .indirect_illum_network .visibility_network
  .envmap_material_network .gamma .rendering_network, forward(), get_idr_render(), assignable get_sg_render,
  trace_radiance().
forward() treats the rays it is given as ONE lock-step batch for the octree tracer, like the reference.

render_chunks(): the same arithmetic for MANY 1024-pixel chunks in one pass -- every kernel sees all chunks at once
(tens of thousands of surface points instead of ~500), while the two chunk-global quantities of the reference
(the octree tracer's active-ray schedule, utils/octree.py:545-549, and the specular-cone minimum,
model/sg_render.py:222) stay per chunk.  Results are what the reference produces rendering the chunks one by one.

Forward only: IDRNetwork.forward runs under no_grad and nothing here differentiates a network.  The SG shading it calls is differentiable
on its own (sg_render.render_with_all_sg with grad mode on, robir_amd/sg_autograd.py): geometry frozen, sampled visibilities constant.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import deferred, dispatch, ops, sg_render
from .precision import cesr_precision, mlp_precision
from .nets import (ImplicitNetworkMy, IndirctIllumNetwork, VisNetwork, EnvmapMaterialNetwork, GammaCorrect,
                   forward_only_guard)
from .octree_tracing import OctreeTracing
from .ray_tracing import RayTracing

TINY_NUMBER = 1e-6
import os as _os
_RANGE_SYNC = _os.environ.get("ROBIR_RANGE_CHECK", "") == "sync"


def _cfg(conf, key):
    sub = conf.get_config(key)
    return {k: sub[k] for k in sub.keys()} if hasattr(sub, "keys") else dict(sub)


_LEGACY_IDR = ("the legacy IDR geometry / appearance networks are built only for use_neus=False, which no shipped configuration sets "
               "(confs_sg/hotdog.conf:68) -- dead code in the reference, OUT OF SCOPE (SURVEY.md section 2 row 1)")


class ImplicitNetwork(nn.Module):
    """model/implicit_differentiable_renderer.py:19-104 (legacy IDR SDF network): present, not built."""

    def __init__(self, feature_vector_size, d_in, d_out, dims, geometric_init=True, bias=1.0, skip_in=(), weight_norm=True, multires=0):
        raise NotImplementedError("ImplicitNetwork: " + _LEGACY_IDR)

    def forward(self, input, compute_grad=False):
        raise NotImplementedError("ImplicitNetwork: " + _LEGACY_IDR)

    def gradient(self, x):
        raise NotImplementedError("ImplicitNetwork: " + _LEGACY_IDR)


class RenderingNetwork(nn.Module):
    """model/implicit_differentiable_renderer.py:107-167 (legacy IDR colour network): present, not built."""

    def __init__(self, feature_vector_size, mode, d_in, d_out, dims, weight_norm=True, multires_view=0):
        raise NotImplementedError("RenderingNetwork (legacy IDR): " + _LEGACY_IDR)

    def forward(self, points, normals, view_dirs, feature_vectors):
        raise NotImplementedError("RenderingNetwork (legacy IDR): " + _LEGACY_IDR)


class IDRNetwork(nn.Module):
    def __init__(self, conf):
        super().__init__()
        if not conf.get_bool("use_neus"):
            raise NotImplementedError("use_neus=False (legacy IDR ImplicitNetwork) is dead in every shipped conf")
        self.feature_vector_size = conf.get_int("feature_vector_size")
        rt = _cfg(conf, "ray_tracer")
        self.octree_ray_tracer = OctreeTracing(**rt, max_iter=32)
        self.use_octree = conf.get_bool("use_octree")
        self.ray_tracer = OctreeTracing(**rt) if self.use_octree else RayTracing(**rt)
        self.object_bounding_sphere = conf.get_float("ray_tracer.object_bounding_sphere")
        self.implicit_network = ImplicitNetworkMy(self.feature_vector_size, **_cfg(conf, "implicit_network"))
        self.rendering_network = self.implicit_network.color
        self.indirect_illum_network = IndirctIllumNetwork(**_cfg(conf, "indirect_illum_network"),
                                                          no_hdr=conf.get_int("hdr_mode") == -1)
        self.visibility_network = VisNetwork(**_cfg(conf, "visibility_network"))
        self.envmap_material_network = EnvmapMaterialNetwork(**_cfg(conf, "envmap_material_network"))
        self.gamma = GammaCorrect(conf.get_float("gamma"), conf.get_int("hdr_mode"))
        self.ray_tracer.bind(self.implicit_network)
        self.octree_ray_tracer.bind(self.implicit_network)
        self.no_normal = False          # PBR hook: use the NeuS normal instead of the Norm-stage normal map
        self.testing = True             # PBR hook's `testing = not is_training`

    # ------------------------------------------------------------------ per-hit pieces
    def get_idr_render(self, points, view_dirs=None, normal_only=False):
        """implicit_differentiable_renderer.py:481-497."""
        g = self.implicit_network.gradient(points)
        normals = g[:, 0, :]
        if normal_only:
            return normals
        feature_vectors = self.implicit_network(points)[:, 1:]
        view_dirs = ops.normalize3(view_dirs.contiguous(), 1e-6, 0)
        return normals, self.rendering_network(points, normals, view_dirs, feature_vectors)

    def batch_idr_forward(self, points, viewdirs, n_pixels=4096):
        """implicit_differentiable_renderer.py:531-546: NeuS radiance of (points, viewdirs) with the L2-normalised SDF gradient as the
        normal -> [M,3].  The reference walks n_pixels rows at a time to bound ITS autograd memory; the rows are independent and the
        kernels are forward-only, so a slab here is max(n_pixels, 2^16) rows (same values)."""
        points, viewdirs = points.float(), viewdirs.float()
        if points.shape[0] == 0:
            return torch.zeros_like(points)
        step = max(int(n_pixels), 1 << 16)
        outs = []
        with torch.no_grad():
            for i in range(0, points.shape[0], step):
                p, v = points[i:i + step].contiguous(), viewdirs[i:i + step].contiguous()
                out, g = self.implicit_network.neus_model.sdf_network.eval_points(p, 2.0, 0.5, full=True, grad=True)
                normals = ops.normalize3(g.contiguous(), TINY_NUMBER, 0)
                outs.append(self.rendering_network(p, normals, v, out[:, 1:]))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def sample_dirs(self, normals, r_theta, r_phi):
        """implicit_differentiable_renderer.py:548-564: directions at polar angle r_phi / azimuth r_theta [num_cam, num_samples] in the
        tangent frame of normals [num_cam, num_samples, 3] (U = norm(x_axis x n), V = norm(n x U)) -> [num_cam, num_samples, 3]."""
        if normals.dim() != 3 or normals.shape[-1] != 3:
            raise ValueError("sample_dirs: normals [num_cam, num_samples, 3]")
        if 3 in normals.shape[:-1]:
            # the reference's torch.cross has no dim=: with a leading size of 3 it crosses along THAT axis (a deprecated torch default)
            raise NotImplementedError("sample_dirs with num_cam == 3 or num_samples == 3: the reference's dim-less torch.cross picks the first "
                                      "axis of size 3, not the vector axis -- not reproduced")
        return ops.sample_dirs(normals.float().contiguous(), r_theta.float().contiguous(), r_phi.float().contiguous()).reshape(normals.shape)

    def get_sg_render(self, points, view_dirs, indir_lgtSGs, albedo_ratio=None, fun_spec=False, lin_diff=False,
                      train_spec=False, indir_integral=None, draws=None, chunk_id=None, n_chunks=1, stats=None, **kwargs):
        """The hook the PBR runner installs (training/train_pbr.py:348-396), restated; the reference's class default
        (implicit_differentiable_renderer.py:499-529) cannot run (KeyError 'metallic')."""
        draws = draws or {}
        vd = ops.normalize3(view_dirs.float().contiguous(), 1e-6, 0)
        normals = ops.normalize3(self.get_idr_render(points, normal_only=True).contiguous(), 1e-4, 1)
        mat = self.envmap_material_network(points, train_spec=True,
                                           noise={"spec": draws.get("spec_randn"), "normal": draws.get("normal_randn")})
        shading_normal = normals if self.no_normal else mat["sg_normal_map"]
        if albedo_ratio is not None:
            # the class default of the reference (implicit_differentiable_renderer.py:508-509): the albedo aligned to ground truth before it
            # is shaded and returned (robir_amd.metrics.albedo_ratio computes the factor).  None: nothing changes.
            mat["sg_diffuse_albedo"] = mat["sg_diffuse_albedo"] * torch.as_tensor(albedo_ratio, dtype=torch.float32,
                                                                                  device=points.device).reshape(1, 3)
        ret = sg_render.render_with_all_sg(points=points, normal=shading_normal, viewdirs=vd, lgtSGs=mat["sg_lgtSGs"],
                                           indir_integral=ops.abs_scale(indir_integral, 2 * np.pi, take_abs=False),
                                           specular_reflectance=mat["sg_specular_reflectance"].abs(),
                                           roughness=mat["sg_roughness"], diffuse_albedo=mat["sg_diffuse_albedo"],
                                           indir_lgtSGs=indir_lgtSGs, VisModel=self.visibility_network, fun_spec=fun_spec,
                                           lin_diff=False, testing=self.testing, metallic=None, draws=draws,
                                           chunk_id=chunk_id, n_chunks=n_chunks, stats=stats)
        ret.update({"normals": normals, "diffuse_albedo": mat["sg_diffuse_albedo"], "roughness": mat["sg_roughness"],
                    "metallic": mat["sg_metallic"], "normal_map": mat["sg_normal_map"],
                    "random_xi_roughness": mat["random_xi_roughness"], "random_xi_metallic": mat["random_xi_metallic"],
                    "random_xi_diffuse_albedo": mat["random_xi_diffuse_albedo"]})
        return ret

    # ------------------------------------------------------------------ forward
    def forward(self, input, trainstage="IDR", fun_spec=False, lin_diff=False, train_spec=False, draws=None, stats=None):
        """implicit_differentiable_renderer.py:290-479, uv/pose/intrinsics input form, batch size 1."""
        forward_only_guard(self)
        # the runner's hook may take per-pixel texture coordinates (implicit_differentiable_renderer.py:390-392,408): kept for _shade,
        # which hands the hit rows to the hook
        self._tex_uv = input.get("tex_uv")
        if "intrinsics" not in input:
            return self._forward_points_dirs(input, trainstage, fun_spec, lin_diff, draws, stats)
        uv, pose, K = input["uv"], input["pose"], input["intrinsics"]
        if uv.shape[0] != 1:
            return self._forward_views(input, trainstage, fun_spec, lin_diff, draws, stats)
        N = uv.shape[1]
        # A call normally is one lock-step chunk, whatever its size (the reference's semantics).  With
        # `model.lockstep_chunk = 1024` a larger call is rendered as consecutive 1024-pixel chunks in one batched pass --
        # the same outputs as the runner's split_input(n_pixels=1024) loop at the batched rate.
        chunk = getattr(self, "lockstep_chunk", None)
        chunk = N if not chunk or N <= chunk else int(chunk)
        limit = self.__dict__.get("deferred_chunks", deferred.DEFAULT_CHUNKS)
        if (limit and not self.training and chunk == N and N <= 1024 and self.use_octree and draws is None and stats is None
                and input.get("albedo_ratio") is None and self._tex_uv is None and not fun_spec
                and not self.indirect_illum_network._trainable()       # a forward that builds a graph runs at once
                and not deferred.hook_trains(self.get_sg_render)):
            rec = self._record_chunk(input, N, int(limit), trainstage, fun_spec, lin_diff)
            if rec is not None:
                return rec
        self.flush()
        return self._render(uv[0], pose[0], K[0], input["object_mask"].reshape(-1), input.get("hdr_shift"), chunk,
                            trainstage, fun_spec, lin_diff, draws, stats, input.get("albedo_ratio"))

    # ------------------------------------------------------------------ deferred chunk forwards (robir_amd/deferred.py)
    def _record_chunk(self, input, N, limit, trainstage, fun_spec, lin_diff):
        uv, pose, K, hdr = input["uv"][0], input["pose"][0], input["intrinsics"][0], input.get("hdr_shift")
        mask = input["object_mask"].reshape(-1)
        hook = self.get_sg_render
        q = self.__dict__.get("_pending")
        if q is not None and (q.seed_epoch != deferred.seed_epoch() or not torch.equal(q.gen.get_state(), q.gen_state)):
            # The caller re-seeded (deferred.seed_epoch: also with the SAME seed, which leaves the state unchanged -- ADVICE r5) or drew
            # random numbers since the pending pass recorded its first chunk: it manages the generator per
            # chunk, and a pass would draw this chunk's numbers from the wrong state.  Run what is pending -- from the state
            # its chunks were recorded under, q.flush() then puts the caller's state back -- and run THIS chunk at once: both are exactly
            # what immediate execution gives.  (None: forward() falls through to the immediate path.)
            q.flush()
            return None
        if q is not None and q.closed:
            # full, or ended by a short chunk: it runs when the NEXT chunk arrives (or at the first read) -- not at its own last forward(),
            # so that a trace_radiance call on that last chunk can still join the pass
            q.flush()
            q = None
        if q is not None:
            psrc, ksrc = q.sig[-2:]
            same = (not q.closed and N <= q.chunk and q.sig[:6] == (trainstage, fun_spec, lin_diff, hdr is None, uv.device, hook)
                    and (psrc == (id(input["pose"]), input["pose"]._version) or torch.equal(pose, q.pose))
                    and (ksrc == (id(input["intrinsics"]), input["intrinsics"]._version) or torch.equal(K, q.K)))
            if not same:
                q.flush()
                q = None
        if q is None:
            sig = (trainstage, fun_spec, lin_diff, hdr is None, uv.device, hook, (id(input["pose"]), input["pose"]._version),
                   (id(input["intrinsics"]), input["intrinsics"]._version))
            spec = deferred.output_spec(trainstage, self.indirect_illum_network.num_lgt_sgs, hdr is not None)
            # pass sizes ramp up: 16, 32, 64, ... `limit` chunks (deferred.RAMP_START) -- the GPU starts after 16 recorded chunks
            ramp = self.__dict__.get("_defer_ramp") or (min(limit, deferred.RAMP_START) if deferred.RAMP_START else limit)
            self.__dict__["_defer_ramp"] = min(limit, 2 * ramp)
            q = deferred.ChunkQueue(self, sig, spec, N, min(limit, ramp), pose, K, hdr is not None, uv.device,
                                    (trainstage, fun_spec, lin_diff, None, None, None))
            # the signature identifies the caller's pose / intrinsics tensors by id(): keep them alive while the queue is, so
            # that a freed tensor's id cannot come back as another view's pose at version 0
            q.sources = (input["pose"], input["intrinsics"])
            self.__dict__["_pending"] = q
        slot = q.add(uv, mask, hdr)
        given = {"object_mask": mask}
        if hdr is not None:
            given["hdr_shift"] = hdr
        return deferred.ChunkOutputs(q, slot, N, uv.device, given)

    def flush(self):
        """Run the recorded chunk forwards, if any (deferred_chunks > 0)."""
        q = self.__dict__.get("_pending")
        if q is not None:
            q.flush()

    def train(self, mode=True):
        deferred.flush_all()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        deferred.flush_all()          # recorded chunk forwards were meant for the weights that are replaced now
        return super().load_state_dict(*args, **kwargs)

    def render_chunks(self, uv, pose, K, hdr_shift, chunk=1024, trainstage="Material", draws=None, stats=None):
        """uv [N,2] for any number of consecutive `chunk`-pixel chunks (chunk <= 1024); pose [4,4], K [3,3];
        hdr_shift [N,1].  draws: dict as synth.pbr_draws but with 'dvis_*' stacked [C,L,32]."""
        forward_only_guard(self)
        self.flush()
        N = uv.shape[0]
        mask = torch.ones(N, dtype=torch.bool, device=uv.device)
        return self._render(uv, pose, K, mask, hdr_shift, chunk, trainstage, False, False, draws, stats, None)

    def _forward_views(self, input, trainstage, fun_spec, lin_diff, draws, stats):
        """Batch size B > 1 (no runner uses it): the reference casts the B x N rays of the B views as ONE lock-step batch from their
        own camera centres and flattens every output to [B N, ...] (implicit_differentiable_renderer.py:299-305,324); every ray is
        traced, `object_mask` only travels along."""
        self.flush()          # a pass recorded by earlier uv-form chunk forwards runs first (it must not stay pending across this call)
        uv, pose, K = input["uv"], input["pose"], input["intrinsics"]
        if pose.dim() == 2 and pose.shape[1] == 7:       # quaternion form, one 7-vector per view (rend_util.py:52-57)
            pose = torch.stack([ops.pose_matrix(pose[b]) for b in range(pose.shape[0])])
        B, N = uv.shape[0], uv.shape[1]
        self.flush()
        with torch.no_grad():
            d = torch.cat([ops.camera_rays(pose[b, :4, :4].float().contiguous(), K[b, :3, :3].float().contiguous(),
                                           uv[b].float().contiguous()) for b in range(B)])
            o = pose[:, None, :3, 3].float().expand(B, N, 3).reshape(-1, 3).contiguous()
        hdr = input.get("hdr_shift")
        return self._render(None, None, None, input["object_mask"].reshape(-1), None if hdr is None else hdr.reshape(B * N, -1),
                            B * N, trainstage, fun_spec, lin_diff, draws, stats, input.get("albedo_ratio"), origins=o, dirs_in=d,
                            trace_all=True)

    def _forward_points_dirs(self, input, trainstage, fun_spec, lin_diff, draws, stats):
        """Second input form (implicit_differentiable_renderer.py:306-322): per-ray origins `points` and directions
        `dirs`; rays outside `object_mask` are not traced (dist 0, no hit).  One lock-step batch."""
        self.flush()          # a pass recorded by earlier uv-form chunk forwards runs first (it must not stay pending across this call)
        o = input["points"].reshape(-1, 3).float()
        d = input["dirs"].reshape(-1, 3).float().contiguous()
        N = o.shape[0]
        mask = input["object_mask"].reshape(-1) if "object_mask" in input else torch.ones(N, dtype=torch.bool, device=o.device)
        return self._render(None, None, None, mask, input.get("hdr_shift"), N, trainstage, fun_spec, lin_diff, draws, stats,
                            input.get("albedo_ratio"), origins=o.contiguous(), dirs_in=d)

    def _render(self, uv, pose, K, object_mask, hdr_shift, chunk, trainstage, fun_spec, lin_diff, draws, stats,
                albedo_ratio, origins=None, dirs_in=None, trace_all=False):
        # split-precision range sentinel (ops.range_check): free of charge without a sync -- an overflow in an earlier call is
        # reported here at the latest; ROBIR_RANGE_CHECK=sync waits for this call's own kernels before returning
        ops.range_check(sync=False)
        out = self._render_impl(uv, pose, K, object_mask, hdr_shift, chunk, trainstage, fun_spec, lin_diff, draws, stats,
                                albedo_ratio, origins, dirs_in, trace_all)
        if _RANGE_SYNC:
            ops.range_check(sync=True)
        return out

    def _render_impl(self, uv, pose, K, object_mask, hdr_shift, chunk, trainstage, fun_spec, lin_diff, draws, stats,
                     albedo_ratio, origins=None, dirs_in=None, trace_all=False):
        draws = draws or {}
        if origins is not None:
            dev, N = origins.device, origins.shape[0]
            with torch.no_grad():
                dirs = dirs_in
                hit = torch.zeros(N, dtype=torch.bool, device=dev)
                dist = torch.zeros(N, device=dev)
                sel = torch.arange(N, device=dev) if trace_all else object_mask.nonzero()[:, 0]
                if sel.numel() > 0 and self.use_octree:
                    _, h, t = self.ray_tracer.sdf_octree.cast_full(origins[sel].contiguous(), dirs[sel].contiguous())
                    hit[sel], dist[sel] = h, t
                elif sel.numel() > 0:
                    _, h, t = self.ray_tracer(sdf=self.implicit_network.sdf_only, cam_loc=origins[sel],
                                              object_mask=object_mask[sel], ray_directions=dirs[sel][:, None, :])
                    hit[sel], dist[sel] = h, t
                n_chunks = 1
                points = ops.points_along(origins, dirs, dist)
                sdf_output = self.implicit_network.sdf_only(points)[:, None]
            return self._shade(points, sdf_output, hit, object_mask, dirs, hdr_shift, chunk, n_chunks, trainstage, fun_spec,
                               lin_diff, draws, stats, albedo_ratio)
        dev = uv.device
        N = uv.shape[0]
        pose = ops.pose_matrix(pose)          # 4x4, or the 7-vector (quaternion | cam_loc) form of get_camera_params (rend_util.py:52-57)
        cam = pose[:3, 3].float().reshape(1, 3).contiguous()
        with torch.no_grad():
            if pose.is_cuda and K.is_cuda:        # read on the device: a .cpu() here would block every per-chunk forward()
                dirs = ops.camera_rays(pose[:4, :4].float().contiguous(), K[:3, :3].float().contiguous(), uv.float().contiguous())
            else:
                dirs = ops.camera_rays(pose.detach().cpu().numpy(), K.detach().cpu().numpy(), uv.float().contiguous())
            if not self.use_octree:       # independent rays: the IDR tracer takes all chunks of the pass at once
                _, hit, dist = self.ray_tracer(sdf=self.implicit_network.sdf_only, cam_loc=cam, object_mask=object_mask,
                                               ray_directions=dirs[None])
                n_chunks = (N + chunk - 1) // chunk
            elif chunk <= 1024:
                _, hit, dist = self.ray_tracer.sdf_octree.cast_chunks(cam, dirs, chunk=chunk)
                n_chunks = (N + chunk - 1) // chunk
            else:
                _, hit, dist = self.ray_tracer(sdf=None, cam_loc=cam, object_mask=object_mask, ray_directions=dirs[None])
                n_chunks = 1
            points = ops.points_along(cam.expand(N, 3).contiguous(), dirs, dist)
            sdf_output = self.implicit_network.sdf_only(points)[:, None]
        return self._shade(points, sdf_output, hit, object_mask, dirs, hdr_shift, chunk, n_chunks, trainstage, fun_spec,
                           lin_diff, draws, stats, albedo_ratio)

    def _shade(self, points, sdf_output, hit, object_mask, dirs, hdr_shift, chunk, n_chunks, trainstage, fun_spec, lin_diff,
               draws, stats, albedo_ratio):
        dev, N = points.device, points.shape[0]
        ret = {"points": points, "sdf_output": sdf_output, "network_object_mask": hit, "object_mask": object_mask,
               "ray_dirs": dirs}
        idx = hit.nonzero()[:, 0]
        n = idx.shape[0]
        hp = points[idx].contiguous()
        cid = (idx // chunk).to(torch.int32).contiguous() if n_chunks > 1 else None
        if cid is not None:
            cid._robir_ascending = True          # idx ascends (pixel order): ops.chunk_ids_ascending need not read it back
        indirect_sgs = torch.ones(N, self.indirect_illum_network.num_lgt_sgs, 7, device=dev)
        indirect_sgs[:, :, -3:] = 0
        indirect_integral = torch.ones(N, 3, device=dev)
        if hdr_shift is not None:
            if n > 0:
                sgs_h, int_h = self.indirect_illum_network(hp, hdr_shift[idx].contiguous(), noise=draws.get("illum_randn"))
                indirect_sgs[idx] = sgs_h
                indirect_integral[idx] = int_h
            ret["hdr_shift"] = hdr_shift
        if trainstage == "Illum":
            normals = torch.ones_like(points)
            if n > 0:
                m = self.envmap_material_network(hp, train_spec=False, train_norm=True,
                                                 noise={"normal": draws.get("normal_randn")})
                normals[idx] = m["sg_normal_map"]
            ret.update({"indirect_sgs": indirect_sgs, "indir_integral": indirect_integral, "normals": normals})
            return ret

        keys3 = ("sg_rgb", "indir_rgb", "sg_diffuse_rgb", "sg_specular_rgb", "indir_diffuse_rgb", "indir_specular_rgb", "normals",
                 "diffuse_albedo", "roughness", "normal_map", "vis_shadow", "random_xi_roughness", "random_xi_diffuse_albedo")
        keys1 = ("metallic", "random_xi_metallic", "acc", "final_t")          # the last two only hold the default
        widths = [3] * len(keys3) + [1] * len(keys1)
        r = None
        bg = None
        gerr = torch.zeros((), device=dev)          # (torch.tensor(0.0, device=...) is a blocking host-to-device copy)
        if self.envmap_material_network.envmap is not None:
            bg = sg_render.render_envmap(self.envmap_material_network.envmap, dirs)
        if n > 0:
            view = (-dirs[idx]).contiguous()
            kw = {}
            if (getattr(self.get_sg_render, "__func__", None) is IDRNetwork.get_sg_render
                    or getattr(self.get_sg_render, "robir_native", False)):
                kw = dict(draws=draws, chunk_id=cid, n_chunks=n_chunks, stats=stats)   # our own hooks understand these
            elif n_chunks > 1:        # a runner's own hook: render_with_all_sg learns the chunk partition from the context
                sg_render._BATCH_CTX = (cid, n_chunks, n)
            tex_uv, self._tex_uv = getattr(self, "_tex_uv", None), None
            if tex_uv is not None:
                if tex_uv.shape[0] * tex_uv.shape[1] == N:          # B views in one batch: rows are (view, pixel) like the hit mask
                    tex_uv = tex_uv.reshape(1, N, *tex_uv.shape[2:])
                if tex_uv.shape[1] != N:
                    raise ValueError("input['tex_uv'] must hold one row per pixel of the call ([B, N, ...], implicit_differentiable_"
                                     "renderer.py:390-392): got %s for %d pixels" % (tuple(tex_uv.shape), N))
                tex_uv = tex_uv[:, hit]
            try:
                r = self.get_sg_render(hp, view, sgs_h if hdr_shift is not None else indirect_sgs[idx],
                                       albedo_ratio=albedo_ratio, fun_spec=fun_spec, lin_diff=lin_diff, train_spec=True,
                                       indir_integral=int_h if hdr_shift is not None else indirect_integral[idx],
                                       tex_uv=tex_uv, hdr_shift=hdr_shift[idx] if hdr_shift is not None else None, **kw)
            finally:
                sg_render._BATCH_CTX = None
            if "gradient_error" in r:
                gerr = gerr + r["gradient_error"]
        # fun_spec (implicit_differentiable_renderer.py:417-427,455-463): the two specular terms come back as functions of a per-pixel
        # roughness; their N-row buffers start as ones and the hit rows are filled in on call
        spec_fn = {}
        if fun_spec and r is not None:
            spec_fn = {k: r[k] for k in ("sg_specular_rgb", "indir_specular_rgb") if callable(r[k])}
        # every output: ones, the hit rows scattered in -- one buffer, one fill, one scatter launch for the seventeen of them
        # (a block without a source has to come last in rb_scatter_rows' view of the buffer: the two function-valued fields scatter ones)
        ones3 = torch.ones(n, 3, device=dev) if spec_fn else None
        srcs = ([ones3 if k in spec_fn else r[k] for k in keys3] + [r["metallic"], r["random_xi_metallic"], None, None]
                if r is not None else [None] * len(widths))
        outs = ops.scatter_rows(srcs + ([None] if bg is None else []), widths + ([3] if bg is None else []), idx, N)
        if bg is None:
            bg = outs.pop()
        ret.update({"gradient_error": gerr, "bg_rgb": bg, "surface_mask": hit})
        ret.update(dict(zip(keys3 + keys1, outs)))
        if r is not None and deferred.hook_trains(self.get_sg_render):
            # a trainable CESR net behind CESRHook: its outputs with a graph go in again by ordinary torch, which carries it.  Every other
            # forward keeps the scatter's graph-free outputs, as before
            for k in keys3:
                if isinstance(r[k], torch.Tensor) and r[k].requires_grad:
                    ret[k] = ret[k].index_put((idx,), r[k].float())
        if fun_spec:
            for k in ("sg_specular_rgb", "indir_specular_rgb"):
                def spec_values_fn(roughness, draws=None, buf=ret[k], fn=spec_fn.get(k)):
                    if fn is not None:      # (draws: explicit uniform draws for the specular cone, robir_amd.sg_render's closures only)
                        buf[idx] = fn(roughness[idx]) if draws is None else fn(roughness[idx], draws=draws)
                    return buf
                ret[k] = spec_values_fn
        return ret

    # ------------------------------------------------------------------ secondary rays
    def trace_radiance(self, input, nsamp=16, test_dir=None, draws=None, chunk=None):
        """implicit_differentiable_renderer.py:566-650.  draws: (u1, u2) uniform [n*nsamp] replacing the two
        torch.rand calls of spherical_uniform.
        chunk: `input` holds several consecutive lock-step chunks of `chunk` pixels (the output of render_chunks): the
        secondary rays of each chunk are then their own lock-step batch (grouped cast), exactly what the reference computes
        calling trace_radiance once per 1024-pixel chunk (training/train_visibility.py); without it the call is ONE batch, like
        one reference call."""
        forward_only_guard(self)
        # a visibility network marked by training.enable_visibility_training, in grad mode: pred_vis carries a graph to its parameters
        # (the scatter below is ordinary torch), so the call runs at once -- a recorded pass runs under no_grad and would drop the graph
        vis_graph = self.visibility_network._trainable()
        if vis_graph:
            self.flush()
        if (not vis_graph and isinstance(input, deferred.ChunkOutputs) and not input._dirty and test_dir is None and draws is None
                and chunk is None):
            # the outputs of a RECORDED chunk forward, default arguments (the runners' per-chunk `trace_radiance(out, nsamp=8)`,
            # training/train_cesr.py:321-326, train_visibility.py): recorded as well -- it runs behind the pass as one grouped call, every
            # chunk its own lock-step batch, with the draws the per-chunk calls would take (robir_amd/deferred.py)
            rec = input._q.record_trace(input._slot, nsamp)
            if rec is not None:
                return rec
        points, shift, mask = input["points"], input["hdr_shift"], input["network_object_mask"]
        dev = points.device
        N = points.shape[0]
        trace = torch.zeros(N, nsamp, 3, device=dev)
        gt_vis = torch.zeros(N, nsamp, 1, dtype=torch.bool, device=dev)
        pred_vis = torch.zeros(N, nsamp, 2, device=dev)
        indir_mask = torch.zeros(N, nsamp, 1, dtype=torch.bool, device=dev)
        gt_int = torch.zeros(N, 3, device=dev)
        idx = mask.nonzero()[:, 0]
        n = idx.shape[0]
        sdirs = torch.zeros(n, nsamp, 3, device=dev)
        if n > 0:
            o = points[idx].contiguous()
            nr = input["normals"].detach()[idx].contiguous()
            if test_dir is not None:
                # one given direction for every sample (implicit_differentiable_renderer.py:594-595): the quantities rb_sphere_dirs
                # derives from its directions, from this one
                nrm = nr / torch.clamp(nr.norm(dim=-1, keepdim=True), min=1e-4)
                d = test_dir.to(dev).float().reshape(1, 3).expand(n * nsamp, 3).contiguous()
                dots = (nrm[:, None, :] * d.view(n, nsamp, 3)).sum(-1)
                back = (dots < 0).reshape(-1).to(torch.uint8).contiguous()
                cosw = torch.relu(dots).reshape(-1).contiguous()
                origins = (o + nrm * 0.005).contiguous()
            else:
                if draws is None:
                    u1, u2 = torch.rand(n * nsamp).to(dev), torch.rand(n * nsamp).to(dev)   # CPU generator, like the reference
                else:
                    u1, u2 = draws
                d, back, cosw, origins = ops.sphere_dirs(u1.to(dev), u2.to(dev), nr, o, nsamp)
            sdirs = d.reshape(n, nsamp, 3)
            with torch.no_grad():
                if chunk is not None and N > chunk:
                    nc = (N + chunk - 1) // chunk
                    per = torch.zeros(nc * chunk, dtype=torch.int64, device=dev)
                    per[:N] = mask.reshape(-1).long()
                    gs = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
                    gs[1:] = torch.cumsum(per.view(nc, chunk).sum(1), 0) * nsamp        # rays of chunk c: gs[c] .. gs[c+1]
                    tree = self.octree_ray_tracer.sdf_octree
                    ro = origins[:, None, :].expand(n, nsamp, 3).reshape(-1, 3).contiguous()
                    sec_x, sec_hit, _ = ops.octree_cast_grouped(tree.tables, ro, sdirs.reshape(-1, 3).contiguous(), gs,
                                                                tree.max_iter)
                else:
                    sec_x, sec_hit, _ = self.octree_ray_tracer(sdf=None, cam_loc=origins, object_mask=None,
                                                               ray_directions=sdirs)
            rad = torch.zeros(n * nsamp, 3, device=dev)
            hidx = sec_hit.nonzero()[:, 0]
            if hidx.numel() > 0:
                col = self.implicit_network.batch_borrow_color(sec_x[hidx].contiguous(), (-d[hidx]).contiguous())
                sh = shift[idx][:, None, :].expand(-1, nsamp, 1).reshape(-1)[hidx].contiguous()
                rad[hidx] = ops.tonemap(col, sh, 2)
            bmask = back.bool()
            rad[bmask] = 0.0
            trace[idx] = rad.reshape(n, nsamp, 3)
            pv = self.visibility_network(o.unsqueeze(1).expand(-1, nsamp, 3).reshape(-1, 3).contiguous(), d)
            pred_vis[idx] = pv.reshape(n, nsamp, 2)
            gt_vis[idx] = sec_hit.reshape(n, nsamp, 1)
            indir_mask[idx] = (~bmask).reshape(n, nsamp, 1) & sec_hit.reshape(n, nsamp, 1)
            gt_int[idx] = ops.trace_integrate(rad, cosw, back, n, nsamp)
        return {"trace_radiance": trace, "sample_dirs": sdirs, "gt_vis": gt_vis, "pred_vis": pred_vis,
                "indir_mask": indir_mask[..., 0], "gt_integral": gt_int}


class CESRHook:
    """ClusteredAlbedoTrainRunner.get_sg_render (training/train_cesr.py:465-544) restated for the HIP path:
    shadow_net evaluated for each of the 128 one-hot light-lobe labels per point, normal_net, linear-diffuse shading
    (`lin_diff=True`) recombined with the albedo.  Install with `model.get_sg_render = CESRHook(model, ...)`."""

    robir_native = True

    def __init__(self, model, shadow_net, normal_net, is_training=False, cur_iter=100000, prefit="explore",
                 argmax_vis=False):
        self.model, self.shadow_net, self.normal_net = model, shadow_net, normal_net
        self.is_training, self.cur_iter, self.prefit, self.argmax_vis = is_training, cur_iter, prefit, argmax_vis

    def __call__(self, points, view_dirs, indir_lgtSGs, albedo_ratio=None, fun_spec=False, lin_diff=False,
                 train_spec=False, indir_integral=None, draws=None, chunk_id=None, n_chunks=1, stats=None, **kwargs):
        m = self.model
        draws = draws or {}
        vd = ops.normalize3(view_dirs.float().contiguous(), 1e-6, 0)
        normals = ops.normalize3(m.get_idr_render(points, normal_only=True).contiguous(), 1e-4, 1)
        mat = m.envmap_material_network(points, train_spec=True,
                                        noise={"spec": draws.get("spec_randn"), "normal": draws.get("normal_randn")})
        x = points.float().contiguous()
        rows = dispatch.cesr(mlp_precision(), cesr_precision(), ops.SDF_FUSED_PE, points=True).encode
        if rows:        # else shadow_net / normal_net straight from the points (encoding inside the kernels)
            x = ops.feat_pe10(x)
        # marked, trainable nets (training.enable_cesr_training): diffuse_vis carries its graph into the shading (rb_sg_shade_bwd hands its
        # gradient back), normal_new into the consistency term below.  The shading takes normal_new DETACHED: it has no gradient with
        # respect to the normal (a deliberate difference from the reference, whose image loss also reaches normal_net)
        diffuse_vis = self.shadow_net.diffuse_vis(x, 128)
        normal_new = self.normal_net.unit_normal(x)
        albedo = mat["sg_diffuse_albedo"]
        ret = sg_render.render_with_all_sg(points=points, normal=normal_new.detach() if self.cur_iter > 1000 else mat["sg_normal_map"],
                                           viewdirs=vd, lgtSGs=mat["sg_lgtSGs"], indir_integral=ops.abs_scale(indir_integral, 2 * np.pi, take_abs=False),
                                           specular_reflectance=mat["sg_specular_reflectance"].abs(),
                                           roughness=mat["sg_roughness"], diffuse_albedo=albedo,
                                           indir_lgtSGs=indir_lgtSGs, VisModel=m.visibility_network, fun_spec=False,
                                           lin_diff=True, testing=not self.is_training, metallic=None,
                                           diffuse_vis=diffuse_vis, prefit=self.prefit, argmax_vis=self.argmax_vis,
                                           draws=draws, chunk_id=chunk_id, n_chunks=n_chunks, stats=stats)
        from .cesr_autograd import lin_diff_combine          # ops.lin_diff_combine; with a graph where an input carries one
        ret["sg_rgb"] = lin_diff_combine(ret["sg_diffuse_rgb"], albedo, ret["sg_specular_rgb"])
        ret["indir_rgb"] = lin_diff_combine(ret["indir_diffuse_rgb"], albedo, ret["indir_specular_rgb"])
        supervise = ret["supervise"] + ((mat["sg_normal_map"] - normal_new) ** 2).mean()
        ret.update({"normals": normals, "diffuse_albedo": albedo, "roughness": mat["sg_roughness"],
                    "metallic": mat["sg_metallic"], "normal_map": normal_new, "gradient_error": supervise,
                    "random_xi_roughness": mat["random_xi_roughness"], "random_xi_metallic": mat["random_xi_metallic"],
                    "random_xi_diffuse_albedo": mat["random_xi_diffuse_albedo"]})
        return ret


class NormHook:
    """NormalTrainRunner.get_sg_render (training/train_normal.py:347-398): no shading in the Norm stage -- NeuS normal,
    materials, the normal map carried in the `diffuse_albedo` slot, constant radiance outputs."""

    robir_native = True

    def __init__(self, model):
        self.model = model

    def __call__(self, points, view_dirs, indir_lgtSGs, albedo_ratio=None, fun_spec=False, lin_diff=False,
                 train_spec=False, indir_integral=None, draws=None, **kwargs):
        draws = draws or {}
        normals = self.model.get_idr_render(points, normal_only=True)              # un-normalised, like the reference
        mat = self.model.envmap_material_network(points, train_spec=True,
                                                 noise={"spec": draws.get("spec_randn"), "normal": draws.get("normal_randn")})
        z, o = torch.zeros_like(points), torch.ones_like(points)
        return {"normals": normals, "sg_rgb": o, "indir_rgb": z, "sg_diffuse_rgb": z, "sg_specular_rgb": z,
                "indir_diffuse_rgb": z, "indir_specular_rgb": z, "vis_shadow": z,
                "diffuse_albedo": mat["sg_normal_map"], "roughness": mat["sg_roughness"], "metallic": mat["sg_metallic"],
                "normal_map": mat["sg_normal_map"], "random_xi_roughness": mat["random_xi_roughness"],
                "random_xi_metallic": mat["random_xi_metallic"], "random_xi_diffuse_albedo": mat["random_xi_normal"]}


# ----------------------------------------------------------------------------------------- construction helpers
class DictConf:
    """Minimal pyhocon-like accessor (get_bool/get_int/get_float/get_config, `**conf.get_config(...)`) so the model
    can be built without pyhocon (tests, bench).  With pyhocon installed the reference's conf objects work as well."""

    def __init__(self, d):
        self.d = d

    def _get(self, key):
        cur = self.d
        for part in key.split("."):
            cur = cur[part]
        return cur

    def get_bool(self, k):
        return bool(self._get(k))

    def get_int(self, k):
        return int(self._get(k))

    def get_float(self, k):
        return float(self._get(k))

    def get_config(self, k):
        return DictConf(self._get(k))

    def keys(self):
        return self.d.keys()

    def __getitem__(self, k):
        return self.d[k]


def hotdog_conf(use_octree=True):
    """model{} section of confs_sg/hotdog.conf:65-123 (truck.conf is identical in this section)."""
    return DictConf({
        "gamma": 1.0, "hdr_mode": 0, "use_neus": True, "use_octree": use_octree, "feature_vector_size": 256,
        "implicit_network": {"d_in": 3, "d_out": 1, "dims": [512] * 8, "geometric_init": True, "bias": 0.6,
                             "skip_in": [4], "weight_norm": True, "multires": 6},
        "rendering_network": {"mode": "idr", "d_in": 9, "d_out": 3, "dims": [512] * 4, "weight_norm": True,
                              "multires_view": 4},
        "indirect_illum_network": {"multires": 10, "dims": [512] * 4, "num_lgt_sgs": 24},
        "visibility_network": {"points_multires": 10, "dirs_multires": 10, "dims": [256] * 4},
        "envmap_material_network": {"multires": 10, "brdf_encoder_dims": [512] * 4, "brdf_decoder_dims": [128, 128],
                                    "num_lgt_sgs": 128, "upper_hemi": False, "specular_albedo": 0.05, "latent_dim": 32},
        "ray_tracer": {"object_bounding_sphere": 1.0, "sdf_threshold": 5.0e-5, "line_search_step": 0.5,
                       "line_step_iters": 3, "sphere_tracing_iters": 10, "n_steps": 100, "n_rootfind_steps": 32},
    })


def build_synthetic_model(device, seed=0, variance=0.3, sharp_light=False, build_octrees=True, use_octree=True, scene="sphere"):
    """IDRNetwork with the synthetic weights of robir_amd.synth (the configuration tests and bench.py use)."""
    from . import synth
    import warnings
    sd = synth.synth_state_dict(seed, variance=variance, sharp_light=sharp_light, scene=scene)
    with warnings.catch_warnings():      # the full state dict is loaded two lines down
        warnings.simplefilter("ignore", RuntimeWarning)
        model = IDRNetwork(hotdog_conf(use_octree))
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    model = model.to(device).eval()
    if build_octrees:
        if use_octree:
            model.ray_tracer.generate(None)
            tree = model.ray_tracer.sdf_octree
            model.octree_ray_tracer.sdf_octree = type(tree)(tree.tables, 32)
        else:                   # secondary rays (trace_radiance) always use the octree tracer, primary rays the IDR tracer
            model.octree_ray_tracer.generate(None)
    return model
