"""Golden vectors for the validation-step metrics: the REFERENCE's own infgen/utils/metrics.py classes (StateAccuracy :485-559,
GridOverlapRate :562-615, minADE :430-467, minFDE :367-390) run on seeded inputs, and torch.nn.CrossEntropyLoss in float64 on the CPU.
Build container only.

    PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION=python python tests/golden/make_golden_valmetrics.py

The stand-in torchmetrics.Metric (_standins.py) has a no-op add_state: every state attribute is set to its default here before
update() is called (float sums as float64 tensors, so that the fixtures hold the float64 value of the reference's arithmetic).
Writes valmetrics_state.npz, valmetrics_grid.npz, valmetrics_traj.npz, valmetrics_ce.npz next to this file.
"""
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
from infgen.utils.metrics import GridOverlapRate, StateAccuracy, minADE, minFDE  # noqa: E402

for _c in (GridOverlapRate, StateAccuracy, minADE, minFDE):
    _standins.assert_reference(_c)

STATE_TOKEN = dict(invalid=0, valid=1, enter=2, exit=3)
I, V, EN, EX = 0, 1, 2, 3
GRID_SIZE, SEED_SIZE = 1961, 4
# the row subsets of the 65-row state matrix: N = 65, 7 and 1 rows (first, one past last)
STATE_SUBSETS = {'n65': (0, 65), 'n7': (3, 10), 'n1': (6, 7)}


def state_rows(T, rng):
    """65 rows: ten special ones, then random sequences"""
    rows = np.zeros((65, T), np.int64)
    rows[0] = rng.choice([I, V], T)                                     # no enter and no exit
    rows[1] = V; rows[1, 0] = EN; rows[1, T - 4] = EX; rows[1, T - 3:] = I      # enter in column 0
    rows[2] = I; rows[2, T - 1] = EN                                    # enter in the last column
    rows[3] = V; rows[3, T - 1] = EX                                    # exit in the last column (wraps to column 0 in part 2)
    rows[4] = V; rows[4, 1] = EX; rows[4, 2:4] = I; rows[4, 4] = EN     # exit before enter
    rows[5] = V; rows[5, 0] = I; rows[5, 1] = EN; rows[5, 3] = EX; rows[5, 4] = I; rows[5, 5] = EN      # two enters
    rows[6] = V; rows[6, 0] = EN; rows[6, 2] = EX; rows[6, 3:6] = I; rows[6, T - 3] = EX; rows[6, T - 2:] = I   # two exits
    rows[7] = I; rows[7, 2] = EN; rows[7, 3] = EX                       # eos == bos + 1
    rows[8] = I                                                         # all invalid
    rows[9] = V                                                         # valid states only
    rows[10:] = rng.choice([I, V, V, V, V, EN, EX], (55, T))
    mask = rng.random((65, T)) > 0.3
    mask[8] = False
    mask[9] = True
    return rows, mask


def run_state(rows, mask):
    m = StateAccuracy(state_token=STATE_TOKEN)
    for k in ('valid', 'valid_count', 'invalid', 'invalid_count'):
        setattr(m, k, torch.tensor(0))
    m.update(state_idx=torch.from_numpy(rows), valid_mask=None if mask is None else torch.from_numpy(mask))
    return np.array([int(m.valid), int(m.valid_count), int(m.invalid), int(m.invalid_count)], np.int64)


def make_state():
    out = {'state_token': np.array([I, V, EN, EX], np.int64)}
    for T in (18, 162):
        rows, mask = state_rows(T, np.random.default_rng(9100 + T))
        out[f't{T}_state'], out[f't{T}_mask'] = rows, mask
        for name, (lo, hi) in STATE_SUBSETS.items():
            out[f't{T}_{name}_rows'] = np.array([lo, hi], np.int64)
            out[f't{T}_{name}_nomask'] = run_state(rows[lo:hi].copy(), None)
            out[f't{T}_{name}_mask'] = run_state(rows[lo:hi].copy(), mask[lo:hi].copy())
    np.savez_compressed(os.path.join(HERE, 'valmetrics_state.npz'), **out)
    print('state', {k: v.tolist() for k, v in out.items() if k.endswith('mask') and v.shape == (4,)})


def run_grid(state, grid, ptr):
    m = GridOverlapRate(num_step=18, state_token=STATE_TOKEN, seed_size=SEED_SIZE)
    keys = ('num_overlap_t', 'num_insert_agent_t', 'num_total_agent_t', 'num_exceed_seed_t')
    for k in keys:
        setattr(m, k, torch.zeros(18).long())
    for lo, hi in zip(ptr[:-1], ptr[1:]):                 # the reference scores whatever it is given as one group
        m.update(state_token=torch.from_numpy(state[lo:hi].copy()), grid_index=torch.from_numpy(grid[lo:hi].copy()))
    return np.stack([getattr(m, k).numpy() for k in keys]).astype(np.int64)


def make_grid():
    rng = np.random.default_rng(9200)
    N, T = 40, 18
    state = rng.choice([I, V, V, V, EN, EX], (N, T)).astype(np.int64)
    grid = rng.integers(0, GRID_SIZE, (N, T)).astype(np.int64)
    grid[rng.random((N, T)) < 0.25] = -1
    grid[:, 7:] = np.where(grid[:, 7:] >= 0, grid[:, 7:] % 23, -1)          # crowded steps: many shared cells

    def step(t, cells, states):
        grid[:, t], state[:, t] = -1, V
        grid[:len(cells), t], state[:len(cells), t] = cells, states
    step(0, [0, 0, 31, 32, 32, 1960, 1960, 31], [EN, V, EN, EN, EX, EN, EN, I])   # the bitmap's word boundaries and last cell
    step(1, [500, 500, 7], [EN, EN, V])                                       # two inserted rows in one free cell
    step(2, [77, 77, 9], [V, EN, EN])                                         # an inserted row on an occupied cell
    step(3, [1234, 1234, 1234], [EN, EN, EN])                                 # three inserted rows in one cell
    step(4, [], [])                                                           # every row at -1
    step(5, [1, 2, 3, 4, 5], [EN, EN, EN, EN, V])                             # n_insert == seed_size
    step(6, [1, 2, 3, 4, 5], [EN, EN, EN, V, V])                              # n_insert == seed_size - 1
    ptr3 = np.array([0, 13, 13, 40], np.int64)                                # three ragged groups, one of them empty
    np.savez_compressed(os.path.join(HERE, 'valmetrics_grid.npz'), state=state, grid=grid, ptr3=ptr3,
                        enter_state=np.int64(EN), seed_size=np.int64(SEED_SIZE), grid_size=np.int64(GRID_SIZE),
                        out_one=run_grid(state, grid, np.array([0, N])), out_groups=run_grid(state, grid, ptr3))
    print('grid overlap', run_grid(state, grid, np.array([0, N]))[0].tolist())


def run_traj(pred, target, valid):
    p, q, v = torch.from_numpy(pred).double(), torch.from_numpy(target).double(), torch.from_numpy(valid)
    res = []
    for cls in (minADE, minFDE):
        m = cls(max_guesses=1)
        m.sum, m.count = torch.tensor(0.0, dtype=torch.float64), torch.tensor(0)
        m.update(pred=p, target=q, valid_mask=v)
        res += [float(m.sum), int(m.count)]
    return res


def make_traj():
    out = {}
    for T, N, seed in ((5, 9, 9301), (91, 70, 9302)):
        rng = np.random.default_rng(seed)
        target = np.cumsum(rng.normal(0, 1.0, (N, T, 2)), 1).astype(np.float32)
        pred = (target + rng.normal(0, 0.7, (N, T, 2))).astype(np.float32)
        valid = rng.random((N, T)) > 0.3
        valid[1] = False                                            # rows with no valid column
        valid[N - 1] = False
        valid[2] = True
        a, ca, f, cf = run_traj(pred, target, valid)
        out.update({f't{T}_pred': pred, f't{T}_target': target, f't{T}_valid': valid, f't{T}_ade_sum': np.float64(a),
                    f't{T}_ade_count': np.int64(ca), f't{T}_fde_sum': np.float64(f), f't{T}_fde_count': np.int64(cf)})
    np.savez_compressed(os.path.join(HERE, 'valmetrics_traj.npz'), **out)
    print('traj', {k: float(v) for k, v in out.items() if v.shape == ()})


def make_ce():
    """logits [R, C] = a u^T + b v^T in float32 (the fixture holds the factors: tests/val_metrics_ref.expand_logits)"""
    out = {}
    cases = {'c4_r300': (4, 300, 0.0, True, 0.5), 'c4_r1': (4, 1, 0.0, True, 0.0), 'c2048_r300': (2048, 300, 0.1, False, 0.5),
             'c2048_r1': (2048, 1, 0.1, False, 0.0), 'c4_allmasked': (4, 5, 0.0, True, 1.0)}
    for i, (name, (C, R, eps, weighted, p_masked)) in enumerate(cases.items()):
        rng = np.random.default_rng(9400 + i)
        a, b = rng.normal(0, 2.0, R).astype(np.float32), rng.normal(0, 1.0, R).astype(np.float32)
        u, v = rng.normal(0, 1.0, C).astype(np.float32), rng.normal(0, 1.0, C).astype(np.float32)
        if R >= 300:
            a[0], b[0] = np.float32(80.0 / np.abs(u).max()), 0.0            # one row spread over +-80 (the log-sum-exp range)
        logits = (a[:, None] * u[None, :]) + (b[:, None] * v[None, :])
        assert logits.dtype == np.float32
        target = rng.integers(0, C, R).astype(np.int64)
        mask = rng.random(R) >= p_masked
        if R >= 300:
            mask[0] = True
        weight = rng.uniform(0.2, 3.0, C).astype(np.float32) if weighted else None
        x, y = torch.from_numpy(logits).double()[torch.from_numpy(mask)], torch.from_numpy(target)[torch.from_numpy(mask)]
        w64 = None if weight is None else torch.from_numpy(weight).double()
        loss = torch.nn.CrossEntropyLoss(weight=w64, label_smoothing=eps)(x, y)
        lp = -torch.log_softmax(x, 1)
        wc = torch.ones(C, dtype=torch.float64) if w64 is None else w64
        sums = np.array([float((wc[y] * lp[torch.arange(len(y)), y]).sum()), float((lp * wc[None]).sum()), float(wc[y].sum())])
        out.update({f'{name}_a': a, f'{name}_u': u, f'{name}_b': b, f'{name}_v': v, f'{name}_target': target, f'{name}_mask': mask,
                    f'{name}_eps': np.float64(eps), f'{name}_loss': np.float64(float(loss)), f'{name}_sums': sums})
        if weight is not None:
            out[f'{name}_weight'] = weight
        print('ce', name, float(loss), int(mask.sum()))
    np.savez_compressed(os.path.join(HERE, 'valmetrics_ce.npz'), **out)


if __name__ == '__main__':
    with torch.no_grad():
        make_state()
        make_grid()
        make_traj()
        make_ce()
