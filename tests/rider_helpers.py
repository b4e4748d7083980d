"""What the GPU tests of the step riders (collision masks, road masks, step scores) share: tensors on the device, an engine on a
fixture, and the check that every emitted token lies in its row's set."""
import numpy as np
import torch

import collision_ref as cr

DEV = 'cuda:0'


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _weights(c, cfg=None):
    from infgen_amd import engine
    return engine.PackedWeights(c['sd'], cfg or c['cfg'], torch.device(DEV))


def _make(c, w, scenes=None, **kw):
    from infgen_amd import engine
    return engine.RolloutEngine(w, scenes or [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw)


def _emitted_in_sets(eng, col, bits, skip=None):
    """every generated live row's token of column col + 1 lies in its set of column col; -> rows checked"""
    K = eng.cfg.token_size
    sets = cr.unpack(bits.cpu().numpy(), K).reshape(eng.S, eng.A_cap, K)
    tok = eng.token[:, col + 1].cpu().numpy()
    st0, st1 = eng.state[:, col].cpu().numpy(), eng.state[:, col + 1].cpu().numpy()
    n = 0
    for s in range(eng.S):
        for r in range(eng.A_cap):
            if st0[s, r] == 0 or st1[s, r] == 0 or tok[s, r] < 0 or (skip is not None and skip[s, r]):
                continue
            assert sets[s, r, tok[s, r]], (s, r, col, int(tok[s, r]))
            n += 1
    return n
