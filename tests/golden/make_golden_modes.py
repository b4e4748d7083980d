"""Golden vectors for the mode selection and the multi-modal errors: the REFERENCE's own infgen/utils/metrics.py - batch_nms
(:198-256), new_batch_nms (:143-195), minMultiFDE.update (:349-361), minMultiADE.update (:403-424; both criteria, with and
without prob, both keep_invalid_final_step values) - run on seeded inputs.  Build container only.

    PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION=python python tests/golden/make_golden_modes.py

Before anything is written the script asserts the conditions under which the reference itself is unambiguous: the scores given
to batch_nms and every prob row are pairwise distinct, no goal distance lies within a relative 1e-5 of dist_thresh (float64),
and no two guesses of a row have equal final or average errors.  new_batch_nms' density scores tie unavoidably: its cases are
well-separated clusters (diameter < dist_thresh / 2, gaps > 4 dist_thresh, pairwise distinct sizes), whose picks are
determined up to the member of the cluster; the cluster labels are part of the fixture.
The metric sums are recorded twice: the reference's arithmetic on float64 copies of the inputs (`*_sum64`) and on the float32
inputs as they are (`*_sum32`: the reference's own float32 error is the yardstick of the device's).
Writes modes_nms.npz, modes_density.npz, modes_multi.npz next to this file (inputs and outputs only)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import _standins  # noqa: E402

_standins.install()
sys.path.insert(0, '/root/reference')
from infgen.utils.metrics import batch_nms, minMultiADE, minMultiFDE, new_batch_nms  # noqa: E402

for _c in (batch_nms, new_batch_nms, minMultiADE, minMultiFDE):
    _standins.assert_reference(_c)

# name: B, N, T, F, K, dist_thresh, seed
NMS_CASES = {'b5_n33': (5, 33, 7, 7, 6, 2.5, 9501), 'b3_n64': (3, 64, 1, 2, 16, 2.5, 9502), 'b4_n6': (4, 6, 7, 2, 6, 1.0, 9503),
             'b2_n2': (2, 2, 7, 2, 1, 2.5, 9504), 'b1_n1': (1, 1, 1, 2, 1, 2.5, 9505), 'b257_n16': (257, 16, 1, 2, 6, 2.5, 9506)}
# name: cluster sizes, K, T, F, dist_thresh, B, seed
DENSITY_CASES = {'n33': ((12, 9, 6, 4, 2), 5, 7, 2, 2.5, 5, 9601), 'n64': ((20, 15, 11, 8, 6, 3, 1), 6, 1, 7, 2.5, 3, 9602),
                 'n33_k8': ((12, 9, 6, 4, 2), 8, 7, 2, 1.0, 2, 9603)}
# name: N, M, T, seed
MULTI_CASES = {'n1_m1_t1': (1, 1, 1, 9701), 'n3_m6_t5': (3, 6, 5, 9702), 'n300_m8_t5': (300, 8, 5, 9703), 'n3_m8_t1': (3, 8, 1, 9704),
               'n300_m1_t5': (300, 1, 5, 9705)}
MAX_GUESSES = 6


def _distinct(rows):
    return all(len(np.unique(r)) == len(r) for r in rows)


def _far_from_threshold(goals, thr):
    g = goals.astype(np.float64)
    d = np.sqrt(((g[:, :, None] - g[:, None, :]) ** 2).sum(-1))
    return not (np.abs(d - thr) <= 1e-5 * thr).any()


def make_nms():
    out = {}
    for name, (B, N, T, F, K, thr, seed) in NMS_CASES.items():
        rng = np.random.default_rng(seed)
        trajs = rng.normal(0, 3.0, (B, N, T, F)).astype(np.float32)
        scores = rng.uniform(0.01, 1.0, (B, N)).astype(np.float32)
        assert _distinct(scores), name
        assert _far_from_threshold(trajs[:, :, -1, :2], thr), name
        rt, rs, ri = batch_nms(torch.from_numpy(trajs), torch.from_numpy(scores), thr, num_ret_modes=K)
        out.update({f'{name}_trajs': trajs, f'{name}_scores': scores, f'{name}_thresh': np.float64(thr), f'{name}_k': np.int64(K),
                    f'{name}_ret_trajs': rt.numpy(), f'{name}_ret_scores': rs.numpy(), f'{name}_ret_idxs': ri.numpy()})
        print('nms', name, ri[0].tolist())
    np.savez_compressed(os.path.join(HERE, 'modes_nms.npz'), **out)


def make_density():
    out = {}
    for name, (sizes, K, T, F, thr, B, seed) in DENSITY_CASES.items():
        rng = np.random.default_rng(seed)
        N = sum(sizes)
        assert len(set(sizes)) == len(sizes)
        trajs = rng.normal(0, 3.0, (B, N, T, F)).astype(np.float32)
        label = np.zeros((B, N), np.int64)
        for b in range(B):
            lab = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
            centre = np.stack([np.arange(len(sizes)) * 6.0 * thr, rng.uniform(-1, 1, len(sizes))], -1)[rng.permutation(len(sizes))]
            ang, rad = rng.uniform(0, 2 * np.pi, N), rng.uniform(0, 0.2 * thr, N)
            trajs[b, :, -1, 0] = (centre[lab, 0] + rad * np.cos(ang)).astype(np.float32)
            trajs[b, :, -1, 1] = (centre[lab, 1] + rad * np.sin(ang)).astype(np.float32)
            label[b] = lab
        g = trajs[:, :, -1, :2].astype(np.float64)
        d = np.sqrt(((g[:, :, None] - g[:, None, :]) ** 2).sum(-1))
        same = label[:, :, None] == label[:, None, :]
        assert d[same].max() < thr / 2 and d[~same].min() > 4 * thr, name
        rt, rs, ri = new_batch_nms(torch.from_numpy(trajs), thr, num_ret_modes=K)
        out.update({f'{name}_trajs': trajs, f'{name}_label': label, f'{name}_thresh': np.float64(thr), f'{name}_k': np.int64(K),
                    f'{name}_ret_scores': rs.numpy(), f'{name}_ret_idxs': ri.numpy()})
        print('density', name, rs[0].tolist())
    np.savez_compressed(os.path.join(HERE, 'modes_density.npz'), **out)


def _guess_errors(pred, target, prob, valid, G):
    p, q = pred.astype(np.float64), target.astype(np.float64)
    for r in range(p.shape[0]):
        if not valid[r].any():
            continue
        M = p.shape[1]
        g = np.arange(min(G, M)) if prob is None or G >= M else np.argsort(-prob[r].astype(np.float64), kind='stable')[:G]
        d = np.sqrt(((p[r, g] - q[r][None]) ** 2).sum(-1))
        yield d[:, np.flatnonzero(valid[r])[-1]], (d * valid[r][None]).sum(-1) / valid[r].sum()


def _run(cls, dtype, pred, target, prob, valid, **kw):
    m = cls(max_guesses=MAX_GUESSES)
    m.device = torch.device('cpu')
    m.sum, m.count = torch.tensor(0.0, dtype=dtype), torch.tensor(0)
    m.update(pred=torch.from_numpy(pred).to(dtype), target=torch.from_numpy(target).to(dtype),
             prob=None if prob is None else torch.from_numpy(prob), valid_mask=torch.from_numpy(valid), **kw)
    return float(m.sum), int(m.count)


def make_multi():
    out = {}
    for name, (N, M, T, seed) in MULTI_CASES.items():
        rng = np.random.default_rng(seed)
        target = np.cumsum(rng.normal(0, 1.0, (N, T, 2)), 1).astype(np.float32)
        pred = (target[:, None] + rng.normal(0, 0.7, (N, M, T, 2))).astype(np.float32)
        prob = rng.uniform(0.05, 1.0, (N, M)).astype(np.float32)
        valid = rng.random((N, T)) > 0.3
        if N >= 3:
            valid[1] = False                                        # a row with no valid step
            valid[2] = False; valid[2, 0] = True                    # a row whose only valid step is the first
            valid[0] = True
        else:
            valid[:] = True
        assert _distinct(prob), name
        for pr in (None, prob):
            for f, a in _guess_errors(pred, target, pr, valid, MAX_GUESSES):
                assert len(np.unique(f)) == len(f) and len(np.unique(a)) == len(a), name
        out.update({f'{name}_pred': pred, f'{name}_target': target, f'{name}_prob': prob, f'{name}_valid': valid})
        for with_prob in (0, 1):
            for keep in (0, 1):
                pr = prob if with_prob else None
                key = f'{name}_p{with_prob}_k{keep}'
                for tag, cls, kw in (('fde', minMultiFDE, {}), ('ade_fde', minMultiADE, dict(min_criterion='FDE')),
                                     ('ade_ade', minMultiADE, dict(min_criterion='ADE'))):
                    s64, c = _run(cls, torch.float64, pred, target, pr, valid, keep_invalid_final_step=bool(keep), **kw)
                    s32, c32 = _run(cls, torch.float32, pred, target, pr, valid, keep_invalid_final_step=bool(keep), **kw)
                    assert c == c32
                    out.update({f'{key}_{tag}_sum64': np.float64(s64), f'{key}_{tag}_sum32': np.float64(s32),
                                f'{key}_{tag}_count': np.int64(c)})
        print('multi', name, float(out[f'{name}_p1_k1_fde_sum64']), int(out[f'{name}_p1_k1_fde_count']))
    out['max_guesses'] = np.int64(MAX_GUESSES)
    np.savez_compressed(os.path.join(HERE, 'modes_multi.npz'), **out)


if __name__ == '__main__':
    with torch.no_grad():
        make_nms()
        make_density()
        make_multi()
