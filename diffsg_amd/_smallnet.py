"""What the two small-net baselines (mtfnn.py, ppo.py) share on the host: tensors and library calls, the flat parameter vector,
the replica list of `fit`, the epoch schedule and permutations, the reference's log sums and the drivers' closing steps.

`module` arguments are the caller's name ("mtfnn" | "ppo"): an error says which baseline raised it."""
from collections import Counter

import numpy as np
import torch
import torch.utils.data as data

from . import _lib


def device():
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: this build of DiffSG has no CPU path")
    return torch.device("cuda:0")


def cuda(module, t, device, what):
    """t as a contiguous float32 (rows, columns) tensor on `device`, which must be a HIP device."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    t = t.detach().to(device=device, dtype=torch.float32).contiguous()
    if not t.is_cuda:
        raise RuntimeError(f"diffsg_amd.{module}.{what}: tensors are not on a HIP device; libdiffsg_hip has no CPU path")
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a (rows, columns) tensor, got {tuple(t.shape)}")
    return t


def call(name, dev, *args):
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr()))


def flat_params(model):
    """The parameters as one flat float32 vector in state-dict order."""
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(torch.float32).contiguous()


def unflatten_into(model, flat):
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()


def named_grads(model, flat):
    """{parameter name: its slice of a flat gradient, shaped as the parameter}."""
    grads, off = {}, 0
    for name, p in model.named_parameters():
        grads[name] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return grads


def cached_flat(model, desc_of):
    """(desc_of(model), flat parameters), rebuilt only after a parameter changed (in-place writes bump a tensor's version, a move to
    another device changes its address): a repeated no-grad forward is then the library launch alone."""
    key = tuple((p.data_ptr(), p._version) for p in model.parameters())
    hit = model.__dict__.get("_dsg_flat")
    if hit is None or hit[0] != key:
        hit = (key, desc_of(model), flat_params(model))
        model.__dict__["_dsg_flat"] = hit
    return hit[1], hit[2]


def replica_list(module, noun, model, replicas, dev, desc_of):
    """The models `fit` trains: `replicas` (with `model` among them) or `model` alone, on the HIP device `dev`, all with `model`'s
    descriptor (compared field by field: a fresh ctypes structure has no stray bytes)."""
    models = list(replicas) if replicas else [model]
    if not any(m is model for m in models):
        raise ValueError(f"fit: `replicas` is the whole list of {noun}s to train and must contain `{noun}`")
    if dev.type != "cuda":
        raise RuntimeError(f"diffsg_amd.{module}.fit: the {noun} is not on a HIP device; libdiffsg_hip has no CPU path")
    if any(bytes(desc_of(m)) != bytes(desc_of(model)) for m in models):
        raise ValueError("fit: the replicas are not of one architecture")
    return models


def epoch_lrs(lr, milestones, epochs, gamma=0.1):
    """The learning rate of every epoch as torch's MultiStepLR yields it: multiplied by gamma ** (times the epoch is listed) when
    the epoch count reaches a milestone -- the chained products, not lr * gamma ** k, so the doubles are the scheduler's."""
    count = Counter(milestones)
    out, cur = [], float(lr)
    for e in range(epochs):
        if e in count:
            cur = cur * gamma ** count[e]
        out.append(cur)
    return out


class _Indices(data.Dataset):
    """arange(n) as a dataset that hands a batch of indices back in one call (the loader's sampler and generator use are those of a
    DataLoader over TensorDataset(arange(n)); only the per-sample fetch, 40 000 tensor reads per epoch, is left out)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i

    def __getitems__(self, idx):
        return idx


def epoch_permutation(n, batch_size):
    """The row order of one epoch: a shuffling DataLoader iterated once, as the reference's `for x, y in data_loader` does, so torch's
    global generator is consumed exactly as there (the iterator's base seed, then the sampler's seed)."""
    loader = data.DataLoader(_Indices(n), batch_size=batch_size, shuffle=True, collate_fn=torch.as_tensor)
    return torch.cat(list(loader)) if n else torch.empty(0, dtype=torch.int64)


def running_sum(values):
    """The reference's `epoch_x += x.item()` over an epoch's batches, in its order and from its integer zero."""
    total = 0
    for v in values:
        total += v
    return total


def figures(pred, true, tag, out):
    out[f"sum_ratio_{tag}"] = float(torch.sum(pred) / torch.sum(true))
    out[f"mean_diff_{tag}"] = float(torch.mean(pred - true))


def finish(model, out, save_path, log):
    if save_path is not None:
        torch.save(model.state_dict(), save_path)
    if log is not None:
        log(", ".join(f"{k}: {v}" for k, v in out.items() if not k.startswith("history")))
    return model, out
