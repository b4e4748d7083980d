"""Validation-step bookkeeping on the device against the reference's per-agent loop, on the same device tensors:
one StateAccuracy.update + GridOverlapRate.update + masked_cross_entropy (infgen_amd/utils/metrics.py) on a
512-scene x 64-agent x 18-column batch with 2048-way logits, and a torch restatement of infgen/utils/metrics.py:499-543,
:574-591 and of ``cross_entropy(pred[mask], gt[mask])``.  Medians of alternating samples (device, reference, device, ...), each
bracketed by a device synchronisation.  Also measures, on the fixtures of tests/golden/, the float kernels' error against the
fixtures' float64 value and the error of the reference's float32 evaluation (the bar of tests/test_val_metrics_gpu.py).

    python tools/bench_val_metrics.py [--scenes 512] [--samples 3] [--out profiles/bench_val_metrics.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
ST = dict(invalid=0, valid=1, enter=2, exit=3)


def ref_state_accuracy(state_idx, st=ST):
    """infgen/utils/metrics.py:499-520 as written (part 1: the closed-loop call has no valid_mask) -> four device scalars"""
    valid = valid_count = invalid = invalid_count = torch.zeros((), dtype=torch.long, device=state_idx.device)
    num_agent, num_step = state_idx.shape
    for a in range(num_agent):
        bos_idx = torch.where(state_idx[a] == st['enter'])[0]
        eos_idx = torch.where(state_idx[a] == st['exit'])[0]
        bos, eos = 0, num_step - 1
        if len(bos_idx) > 0:
            bos = bos_idx[0]
            invalid = invalid + (state_idx[a, :bos] == st['invalid']).sum()
            invalid_count = invalid_count + len(state_idx[a, :bos])
        if len(eos_idx) > 0:
            eos = eos_idx[0]
            invalid = invalid + (state_idx[a, eos + 1:] == st['invalid']).sum()
            invalid_count = invalid_count + len(state_idx[a, eos + 1:])
        valid = valid + (state_idx[a, bos + 1: eos] == st['valid']).sum()
        valid_count = valid_count + len(state_idx[a, bos + 1: eos])
    return torch.stack([valid, valid_count, invalid, invalid_count])


def ref_grid_overlap(state_token, grid_index, num_step, seed_size, st=ST):
    """infgen/utils/metrics.py:574-591 as written -> [4, num_step] (host lists, like the reference)"""
    out = np.zeros((4, num_step), np.int64)
    for t in range(num_step):
        inrange = grid_index[:, t] != -1
        insert = (state_token[:, t] == st['enter']) & inrange
        out[2, t] += int(inrange.sum())
        out[1, t] += int(insert.sum())
        out[3, t] += int(insert.sum() >= seed_size)
        occupied = set(grid_index[:, t][(grid_index[:, t] != -1) & (state_token[:, t] != st['enter'])].tolist())
        todo = grid_index[:, t][(grid_index[:, t] != -1) & (state_token[:, t] == st['enter'])].tolist()
        while todo:
            g = todo.pop()
            if g in occupied:
                out[0, t] += 1
            occupied.add(g)
    return out


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def error_ratios(dev):
    """device error / float32-reference error on the fixtures (float64 value = the fixture's)"""
    import val_metrics_ref as R
    from infgen_amd.utils.metrics import masked_cross_entropy, minADE, minFDE
    golden = os.path.join(REPO, 'tests', 'golden')
    out = {}
    t = np.load(os.path.join(golden, 'valmetrics_traj.npz'))
    for T in (5, 91):
        pn, qn, vn = (t[f't{T}_{k}'] for k in ('pred', 'target', 'valid'))
        p, q, v = (torch.from_numpy(x) for x in (pn, qn, vn))
        E = min(70, T)
        ref32 = dict(ade=float(((torch.norm(p[:, :E] - q[:, :E], p=2, dim=-1) * v[:, :E]).sum(-1) / T).sum()),
                     fde=float((torch.norm(p[:, E - 2:E - 1] - q[:, E - 2:E - 1], p=2, dim=-1) * v[:, E - 2].unsqueeze(1)).sum()))
        for k, cls in (('ade', minADE), ('fde', minFDE)):
            m = cls(max_guesses=1)
            m.update(pred=p.to(dev), target=q.to(dev), valid_mask=v.to(dev))
            got, ref64 = float(m.state()['buf'].view(torch.float64)[0]), float(t[f't{T}_{k}_sum'])
            out[f'traj_t{T}_{k}'] = dict(device_err=abs(got - ref64), float32_err=abs(ref32[k] - ref64))
    c = np.load(os.path.join(golden, 'valmetrics_ce.npz'))
    for name in ('c4_r300', 'c4_r1', 'c2048_r300', 'c2048_r1'):
        xn = R.expand_logits(c[name + '_a'], c[name + '_u'], c[name + '_b'], c[name + '_v'])
        wn = c[name + '_weight'] if name + '_weight' in c.files else None
        eps, mt = float(c[name + '_eps']), torch.from_numpy(c[name + '_mask'])
        ref32 = float(torch.nn.CrossEntropyLoss(weight=None if wn is None else torch.from_numpy(wn), label_smoothing=eps)(
            torch.from_numpy(xn)[mt], torch.from_numpy(c[name + '_target'])[mt]))
        got = float(masked_cross_entropy(torch.from_numpy(xn).to(dev), torch.from_numpy(c[name + '_target']).to(dev), mt.to(dev),
                                         weight=None if wn is None else torch.from_numpy(wn).to(dev), label_smoothing=eps))
        ref64 = float(c[name + '_loss'])
        out[f'ce_{name}'] = dict(device_err=abs(got - ref64), float32_err=abs(ref32 - ref64))
    for v in out.values():
        v['ratio'] = v['device_err'] / v['float32_err'] if v['float32_err'] > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--classes', type=int, default=2048)
    ap.add_argument('--samples', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_val_metrics.json'))
    a = ap.parse_args()
    from infgen_amd.utils.metrics import GridOverlapRate, StateAccuracy, masked_cross_entropy
    dev = torch.device('cuda:0')
    T, N, C = 18, a.scenes * a.agents, a.classes
    g = torch.Generator(device='cpu').manual_seed(1)
    state = torch.randint(0, 8, (N, T), generator=g).clamp(max=5)
    state = torch.tensor([0, 1, 1, 1, 2, 3])[state].to(dev)                      # mostly valid, some enter / exit / invalid
    grid = torch.randint(-1, 1961, (N, T), generator=g).to(dev)
    ptr = torch.arange(0, N + 1, a.agents, device=dev)
    logits = torch.randn(N * T, C, device=dev)
    target = torch.randint(0, C, (N * T,), generator=g).to(dev)
    mask = (torch.rand(N * T, generator=g) < 0.5).to(dev)
    sa = StateAccuracy(state_token=ST)
    go = GridOverlapRate(num_step=T, state_token=ST, seed_size=10, grid_size=1961)

    def device_pass():
        sa.reset(); go.reset()
        sa.update(state_idx=state)
        go.update(state_token=state, grid_index=grid, ptr=ptr)
        return masked_cross_entropy(logits, target, mask, label_smoothing=0.1)

    def reference_pass():
        c = ref_state_accuracy(state)
        o = ref_grid_overlap(state, grid, T, 10)            # (one group, like the reference)
        return c, o, torch.nn.functional.cross_entropy(logits[mask], target[mask], label_smoothing=0.1)

    parts = {'state_accuracy': (lambda: sa.update(state_idx=state), lambda: ref_state_accuracy(state)),
             'grid_overlap': (lambda: go.update(state_token=state, grid_index=grid, ptr=ptr), lambda: ref_grid_overlap(state, grid, T, 10)),
             'cross_entropy': (lambda: masked_cross_entropy(logits, target, mask, label_smoothing=0.1),
                               lambda: torch.nn.functional.cross_entropy(logits[mask], target[mask], label_smoothing=0.1))}
    device_pass()                                            # warm-up: library load, allocator
    torch.nn.functional.cross_entropy(logits[mask], target[mask], label_smoothing=0.1)
    d_ms, r_ms, part_ms = [], [], {k: ([], []) for k in parts}
    for _ in range(a.samples):
        ms, loss = timed(device_pass, dev)
        d_ms.append(ms)
        ms, (c_ref, o_ref, loss_ref) = timed(reference_pass, dev)
        r_ms.append(ms)
        for k, (fd, fr) in parts.items():
            part_ms[k][0].append(timed(fd, dev)[0])
            part_ms[k][1].append(timed(fr, dev)[0])
    sa.reset()
    sa.update(state_idx=state)
    go1 = GridOverlapRate(num_step=T, state_token=ST, seed_size=10, grid_size=1961)
    go1.update(state_token=state, grid_index=grid)
    same = bool(torch.equal(sa.state()['buf'], c_ref)) and bool(np.array_equal(go1.state()['buf'].cpu().numpy().reshape(4, T), o_ref))
    med = statistics.median
    res = dict(tool='tools/bench_val_metrics.py', device=torch.cuda.get_device_name(0), scenes=a.scenes, agents_per_scene=a.agents,
               columns=T, classes=C, rows=N, logit_rows=N * T, samples=a.samples,
               device_ms=round(med(d_ms), 3), reference_ms=round(med(r_ms), 1), device_ms_samples=[round(x, 3) for x in d_ms],
               reference_ms_samples=[round(x, 1) for x in r_ms],
               parts={k: dict(device_ms=round(med(v[0]), 3), reference_ms=round(med(v[1]), 3)) for k, v in part_ms.items()},
               counters_equal_reference=same, loss_device=float(loss), loss_reference_float32=float(loss_ref),
               float_errors=error_ratios(dev))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
