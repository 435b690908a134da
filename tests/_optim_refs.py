"""Independent reference for the SGD / Momentum / RMSProp optimizer steps,
written from the formulas (TF's) in the style of `_fp64_refs.adam_ref`:
evaluated in float64 it is the reference, in float32 on the CPU it gives the
noise floor.  Nothing here imports sat_amd.

    g    = scale * grad,  scale = clip / norm if norm > clip else 1
                          (norm = global l2 norm; clip <= 0: no clipping)
    lr   = lr0 * decay ** floor(t / spd)          (only if decay < 1)
    SGD       p -= lr g
    Momentum  mom = momentum mom + g
              p -= lr mom              or, nesterov,  lr (g + momentum mom)
    RMSProp   ms = rho ms + (1 - rho) g g
              mg = rho mg + (1 - rho) g                       (centered)
              mom = momentum mom + lr g / sqrt(ms [- mg mg] + eps)
              p -= mom
"""

import torch

SLOTS = {'SGD': (), 'Momentum': ('mom',), 'RMSProp': ('ms', 'mom', 'mg')}


def slot_names(kind, hp):
    if kind == 'RMSProp' and not hp['centered']:
        return ('ms', 'mom')
    return SLOTS[kind]


def opt_ref(kind, ps, gs, slots, t, hp, dtype):
    """One step on lists of CPU tensors, all arithmetic in `dtype`.
    slots: {name: list of tensors} with the names of slot_names(kind, hp).
    hp: dict(lr0, decay, spd, clip, momentum, rho, eps, nesterov, centered).
    Returns (new ps, new slots, lr, scale) without touching the inputs."""
    def S(x):
        return torch.tensor(float(x), dtype=dtype)
    names = slot_names(kind, hp)
    ps = [x.to(dtype) for x in ps]
    gs = [x.to(dtype) for x in gs]
    sl = {k: [x.to(dtype) for x in slots[k]] for k in names}
    gsq = sum((g * g).sum() for g in gs)
    norm = gsq.sqrt()
    scale = S(1.0)
    if hp['clip'] > 0 and norm > S(hp['clip']):
        scale = S(hp['clip']) / norm
    lr = S(hp['lr0'])
    if hp['decay'] < 1.0:
        lr = lr * S(hp['decay']) ** torch.floor(S(t) / S(hp['spd']))
    mu, rho, eps = S(hp['momentum']), S(hp['rho']), S(hp['eps'])
    pn = []
    out = {k: [] for k in names}
    for i, (p, g) in enumerate(zip(ps, gs)):
        g = g * scale
        if kind == 'SGD':
            pn.append(p - lr * g)
        elif kind == 'Momentum':
            mom = mu * sl['mom'][i] + g
            out['mom'].append(mom)
            if hp['nesterov']:
                pn.append(p - lr * (g + mu * mom))
            else:
                pn.append(p - lr * mom)
        elif kind == 'RMSProp':
            ms = rho * sl['ms'][i] + (1 - rho) * g * g
            out['ms'].append(ms)
            den = ms
            if hp['centered']:
                mg = rho * sl['mg'][i] + (1 - rho) * g
                out['mg'].append(mg)
                den = den - mg * mg
            mom = mu * sl['mom'][i] + lr * g / (den + eps).sqrt()
            out['mom'].append(mom)
            pn.append(p - mom)
        else:
            raise ValueError(kind)
    return pn, out, lr.item(), scale.item()
