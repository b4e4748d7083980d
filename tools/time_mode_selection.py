"""Timing of the mode selection (``RolloutEngine.select_modes``, k_select_modes); bench.py is untouched.

    python tools/time_mode_selection.py [--samples 21] [--log profiles/mode_selection.log]

Set-up: 32 C3 scenes x 32 copies (64 agents, 1024 map tokens, R = 80), ``sample_k = 5``, K = 6, dist_thresh = 2.5, one sampled
rollout; both variants then read the same ``pred_traj`` on the device.  Between HIP events, alternating A B A B ... so that drift
of the machine lands on both alike; medians (and the spread) are reported:

    (a) select_modes   ``RolloutEngine.select_modes(k=6)`` with given scores: pred_traj read in place, one launch plus mode_prob
    (a') density       the same with scores='density'
    (b) torch          the reference's batch_nms algorithm written with torch ops (tests/modes_ref.batch_nms_torch) on the same
                       candidates as a [S0 * A_cap, copies, R, 2] view - with the permuted copy the reference's layout needs
                       counted (b) and not counted (b'), since a caller holding the engine's layout has to make it
The picks of (a) and (b) are compared where every candidate is valid (the torch form has no validity mask)."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=21)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    import json
    import numpy as np
    import torch
    import modes_ref
    from infgen_amd import engine, synth
    dev = torch.device('cuda:0')
    with open(os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    S0, N, K, THR = 32, 32, 6, 2.5
    cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
    sd = synth.fill_state_dict(shapes, seed=1, rich=True)
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid)
              for i in range(S0)]
    u = np.random.default_rng(7).random((cfg.num_decode_steps, S0 * N, 64), dtype=np.float32)
    w = engine.PackedWeights(sd, cfg, dev)
    eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=N, sample_k=5, sample_uniforms=u)
    eng.rollout()
    torch.cuda.synchronize(dev)
    A_cap, R = eng.A_cap, eng.R
    scores = torch.rand(S0, N, device=dev) + 0.01
    view = eng.pred_traj.view(S0, N, A_cap, R, 2).permute(0, 2, 1, 3, 4)
    row_scores = scores[:, None, :].expand(S0, A_cap, N).reshape(-1, N).contiguous()
    flat = view.reshape(-1, N, R, 2)                                            # (the permuted copy, made once for b')

    def a():
        return eng.select_modes(k=K, dist_thresh=THR, scores=scores)

    def a_density():
        return eng.select_modes(k=K, dist_thresh=THR, scores='density')

    def b():
        return modes_ref.batch_nms_torch(view.reshape(-1, N, R, 2), row_scores, THR, K)

    def b_nocopy():
        return modes_ref.batch_nms_torch(flat, row_scores, THR, K)

    variants = [('a  select_modes (given scores)', a), ("a' select_modes (density)", a_density), ('b  torch batch_nms incl. layout copy', b),
                ("b' torch batch_nms, layout copy not counted", b_nocopy)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in variants}
    for _ in range(args.samples):
        for name, fn in variants:
            times[name].append(timed(fn))
    ma, mb = a(), b()
    st = eng.pred_state.view(S0, N, A_cap, R)[..., -1]
    valid_rows = ((st != synth.INVALID) & (st != synth.ENTER)).all(dim=1).reshape(-1)
    same = int((ma['mode_idx'].reshape(-1, K)[valid_rows].long() == mb[2][valid_rows]).all(-1).sum())
    lines = [f'mode selection: {S0} scenes x {N} copies, A_cap {A_cap}, R {R}, K {K}, dist_thresh {THR}; {S0 * A_cap} rows, '
             f'{args.samples} alternating samples after {args.warmup} warm-up rounds, HIP events, microseconds',
             f'device: {torch.cuda.get_device_name(dev)}']
    for name, _ in variants:
        t = sorted(times[name])
        lines.append(f'  {name:46s} median {statistics.median(t):9.1f}  min {t[0]:9.1f}  max {t[-1]:9.1f}')
    med = {name: statistics.median(times[name]) for name, _ in variants}
    lines.append(f'  ratio b / a: {med[variants[2][0]] / med[variants[0][0]]:.1f}x    b\' / a: {med[variants[3][0]] / med[variants[0][0]]:.1f}x')
    lines.append(f'  rows whose {N} candidates are all valid: {int(valid_rows.sum())} of {valid_rows.numel()}; picks of (a) and (b) equal '
                 f'in {same} of them')
    lines.append(f'  (a) writes {S0 * A_cap * K * R * 2 * 4 / 1e6:.2f} MB of trajectories; its time includes the host-side launches and mode_prob')
    text = '\n'.join(lines)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
