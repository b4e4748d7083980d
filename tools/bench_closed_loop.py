"""cost of stepping a rollout through a closed-loop session (infgen_amd/closed_loop.py) against ``rollout()`` with the graph off.

    python tools/bench_closed_loop.py [--scenes 1024] [--samples 7] [--warmup 2] [--out profiles/closed_loop.log]

BASELINE C3 shape (64 agents, 1024 map tokens, R = 80, greedy, insertion off).  One engine replays the ego (``replay='ego'``-style
mask); a sample of the session = prologue + 16 x (command kernel + decode step) with the ego's token commands taken from a device
tensor (the tokens the free rollout stored: both legs compute the same scene), a sample of the rollout = ``rollout()`` on a second
engine with the same mask whose plan holds those tokens up front.  Samples alternate; HIP events around each; median and spread of
each leg, and the command kernel alone (events around 16 launches)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                           # noqa: E402
from infgen_amd import _lib, engine, synth                             # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=1024)
    ap.add_argument('--samples', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='append the report to this file too')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
    sd = synth.fill_state_dict(bench.load_shapes(), seed=1, rich=True)
    scenes, vocab, map_vocab, grid = bench.build_scenes(cfg, range(args.scenes), 64, 1024, procs=bench.host_procs(1))
    w = engine.PackedWeights(sd, cfg, dev)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    masks = []
    for sc in scenes:
        keep = np.asarray(sc['agent']['state_idx'])[:, hc - 1] != 0
        m = np.zeros(keep.shape[0], bool)
        m[int(np.asarray(sc['agent']['av_index']).reshape(-1)[0])] = True
        masks.append(m)
    mk = lambda: engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, store_logits=False, use_graph=False, replay=masks)
    free = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, store_logits=False, use_graph=False)
    free.rollout()
    S = free.S
    ar = torch.arange(S, device=dev)
    ego_tok = free.token[ar, :, free.av.long()].T.contiguous()        # [T, S]: the command of step t is row hc + t
    want = int(free.token.long().sum())
    del free
    e_ses, e_roll = mk(), mk()
    # the rollout leg's plan: the same tokens, up front (states valid)
    e_roll.teacher_token[ar, :, e_roll.av.long()] = ego_tok.T
    e_roll.teacher_state[ar, :, e_roll.av.long()] = 1
    if e_roll.teacher_pos is not None:
        e_roll._alloc_replay(False)

    def session():
        ses = e_ses.session()
        while not ses.done:
            ses.command(tokens=ego_tok[hc + ses.t])
            ses.advance()

    for _ in range(args.warmup):
        session(); e_roll.rollout()
    torch.cuda.synchronize()
    same = int(e_ses.token.long().sum()) == int(e_roll.token.long().sum()) == want
    t_ses, t_roll = [], []
    for _ in range(args.samples):
        t_ses.append(timed(session))
        t_roll.append(timed(e_roll.rollout))
    ses = e_ses.session()
    ses.command(tokens=ego_tok[hc])
    P, ctx = _lib.ptr, C.byref(e_ses._ctx)
    st = e_ses.ops.stream
    launch = lambda: [e_ses.lib.infgen_command_rows(ctx, t, 0, P(ses._tok), None, P(ses._mask), None, P(ses.cost), st) for t in range(steps)]
    launch()
    t_cmd = [timed(launch) / steps * 1e3 for _ in range(args.samples)]
    launch_p = lambda: [e_ses.lib.infgen_command_rows(ctx, t, 1, None, P(ses._pose), P(ses._mask), P(e_ses._shape10), P(ses.cost), st)
                        for t in range(steps)]
    launch_p()
    t_cmd_p = [timed(launch_p) / steps * 1e3 for _ in range(args.samples)]
    med = lambda x: float(np.median(x))
    rep = {'scenes': S, 'rows_per_scene': e_ses.A_cap, 'steps': steps, 'samples': args.samples,
           'session_ms': {'median': med(t_ses), 'min': min(t_ses), 'max': max(t_ses)},
           'rollout_ms': {'median': med(t_roll), 'min': min(t_roll), 'max': max(t_roll)},
           'command_kernel_us': {'token': med(t_cmd), 'pose': med(t_cmd_p)},
           'same_tokens_as_the_free_rollout': same, 'session_samples_ms': t_ses, 'rollout_samples_ms': t_roll}
    line = json.dumps(rep)
    print(line)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
