"""Test-side truth for the CESR networks' backward: torch autograd of the oracle's formulas (robir_oracle.nets.softplus_net512, the encoding
robir_oracle.nets.pe) on the CPU, in float64 (the truth) or float32 (the yardstick: what PyTorch's own fp32 autograd achieves on the same
inputs).  The points form evaluates the encoding in the evaluation's dtype from the fp32 coordinates and builds the one-hot block from the row
index; the dense form takes the fp32 rows the kernel saw.  Shared by tests/test_cesr_train_cpu.py, tests/test_cesr_train_gpu.py,
tools/gen_cesr_grad_golden.py and tools/prof_cesr_backward.py."""
import torch

from robir_oracle import nets as on

NAMES = tuple(f"lin{l}.{w}" for l in range(9) for w in ("weight_g", "weight_v", "bias"))      # ops.CESR_PARAM_NAMES
DIMS = {"normal": (63, 3), "shadow": (191, 2)}


def cesr_params(sd):
    """The 27 tensors of one CESR network out of its state dict (robir_amd.synth.synth_cesr_nets()[name]), keyed by NAMES."""
    return {k: torch.as_tensor(sd[k]) for k in NAMES}


def leaves(params, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}


def _dtype(params):
    return next(iter(params.values())).dtype


def rows_of_points(points, n_label, kind, dtype):
    """The rows of the points form: [PE10(points[i / n_label]) | onehot(i % n_label, 128)] (shadow) or PE10(points[i]) (normal), `dtype`."""
    feat = on.pe(points.detach().float().to(dtype), 10)
    if kind == "normal":
        return feat
    n = feat.shape[0]
    hot = torch.zeros(n_label, 128, dtype=dtype)
    hot[torch.arange(n_label), torch.arange(n_label)] = 1
    return torch.cat([feat[:, None, :].expand(n, n_label, 63), hot[None].expand(n, n_label, 128)], -1).reshape(n * n_label, 191)


def head_of(raw, head):
    """0: the raw output; 1: the class-1 probability of the two-class softmax; 2: raw / max(|raw|, 1e-4)."""
    if head == 0:
        return raw
    if head == 1:
        return torch.softmax(raw, -1)[:, 1]
    return raw / torch.clamp(torch.norm(raw, dim=-1, keepdim=True), min=1e-4)


def forward(params, x, kind, n_label=1, head=0):
    """head(softplus_net512(rows)) in the dtype of `params`; x: fp32 points [n,3] (the points form) or fp32 dense rows [M, >= d_in]."""
    dtype = _dtype(params)
    d_in = DIMS[kind][0]
    rows = rows_of_points(x, n_label, kind, dtype) if x.shape[1] == 3 else x.detach().float()[:, :d_in].to(dtype)
    return head_of(on.softplus_net512(params, rows), head)


def grads_of(loss_fn, params, dtype, names=None):
    """(loss value, dict name -> gradient) of loss_fn(leaves) for `names` (default: all 27)."""
    with torch.enable_grad():
        lv = leaves(params, dtype)
        loss = loss_fn(lv)
        keys = list(names or lv)
        gr = torch.autograd.grad(loss, [lv[k] for k in keys])
    return float(loss.detach()), dict(zip(keys, gr))


def grads(params, x, kind, g_out, dtype, n_label=1, head=0, names=None):
    """d <g_out, head(net(x))> / d params in `dtype` from the fp32 inputs."""
    fn = lambda lv: (g_out.detach().float().to(dtype).reshape(-1) * forward(lv, x, kind, n_label, head).reshape(-1)).sum()
    return grads_of(fn, params, dtype, names)[1]
