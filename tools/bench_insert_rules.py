"""Timing and effect of the insertion rules (``insert_rules``, k_insert_cell_mask); bench.py is untouched.

    python tools/bench_insert_rules.py [--parent DIR] [--scenes 1024] [--rounds 3] [--log profiles/insert_rules.log]

C3 scenes (64 agents, 1024 map tokens), scenario insertion on, force_enter.  Every sample is a fresh process; the variants of a
figure alternate A B C A B C ... and medians are reported with their spreads, next to the raw samples.  Figures:

    (a) rollout     one whole rollout (prologue + decode steps, host clock around a device synchronise) with
                        parent    ``--parent`` (a built checkout of the parent commit), no rules; skipped without ``--parent``
                        none      this tree, insert_rules=None: the parent's launches
                        nothing   a rule set that bans nothing (clearance 0, every type, no budget): the mask kernel and the masked
                                  decision run, the outputs are those of ``none``
                        real      clearance 6 m, ego keep-out 5 / 40 / 4 m, near_lane 9 m, vehicles and cyclists, at most 96 live agents,
                                  at most 3 insertions per step
    (b) kernel      ``infgen_insert_cell_mask`` on the final column of that batch between device events: static + clearance (pass 1)
                    and clearance only (pass 2), the realistic rule set
    (c) effect      over the rows the rollout inserted: the share that starts within 6 m (box distance, the rule's own) of another
                    box of its column, and the share with no lane token within 9 m - rules off (``none``) and on (``real``)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAR, LANE = 6.0, 9.0

WORKER = r'''
import json, sys, time
root, variant, scenes_n, shapes_json = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(shapes_json) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=False, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid)
          for i in range(scenes_n)]
CLEAR, LANE, LANE_TYPES = %(clear)r, %(lane)r, tuple(range(0, 12))
rules = dict(none=None, parent=None, nothing=dict(clearance=0.0, types=('veh', 'ped', 'cyc')),
             real=dict(clearance=CLEAR, ego_keepout=(5.0, 40.0, 4.0), near_lane=dict(dist=LANE, types=LANE_TYPES), types=('veh', 'cyc'),
                       max_agents=96, per_step=3))[variant]
kw = {} if variant == 'parent' else dict(insert_rules=rules)
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, force_enter=True, **kw)
eng.rollout(); torch.cuda.synchronize()                       # warm-up: code objects, buffers, edge capacities
t0 = time.perf_counter(); eng.rollout(); torch.cuda.synchronize()
out = dict(variant=variant, rollout_ms=(time.perf_counter() - t0) * 1e3, inserted=int(sum(len(r) for r in eng.ins['inserted_rows'])))
S, A, T = eng.S, eng.A_cap, eng.T
pos, head, state = eng.pos.view(S, T, A, 2), eng.head.view(S, T, A), eng.state.view(S, T, A)
# (c) the inserted rows against the boxes of their column (rows in front of them) and the lane tokens; torch on the device
shape = torch.maximum(eng._shape10.view(S, A, 3), eng.ins['shape_all'].view(S, A, 3))      # (the unused one of the two holds 0.1)
mtype = eng._map_cat[1].view(eng.S0, eng.M_cap)
lane_ok = (torch.arange(eng.M_cap, device=dev)[None] < eng.n_map[:, None]) & (mtype >= 0) & (mtype < 12)
close = nolane = n = 0
for s, rows in enumerate(eng.ins['inserted_rows'][:64]):      # (the first 64 scenes: every row costs two device reads)
    for row, t in rows:
        a, c = row - s * A, 1 + t
        p = pos[s, c, a]
        live = state[s, c, :a] != 0
        d = p[None] - pos[s, c, :a]
        ch, sh = torch.cos(head[s, c, :a]), torch.sin(head[s, c, :a])
        lx, ly = d[:, 0] * ch + d[:, 1] * sh, d[:, 1] * ch - d[:, 0] * sh
        ox = (lx.abs() - 0.5 * shape[s, :a, 0]).clamp(min=0); oy = (ly.abs() - 0.5 * shape[s, :a, 1]).clamp(min=0)
        close += int(((ox * ox + oy * oy).sqrt()[live] < CLEAR).any())
        dm = (eng.map_pos.view(eng.S0, eng.M_cap, 2)[s // eng.copies] - p[None]).norm(dim=1)
        nolane += int(not (dm[lane_ok[s // eng.copies]] <= LANE).any())
        n += 1
out.update(rows=n, share_close=close / max(n, 1), share_no_lane=nolane / max(n, 1))
if variant == 'real':
    # (b) the kernel alone on the final state, between device events
    from infgen_amd import _lib
    P, k, c = _lib.ptr, eng._ins_rules, T - 2
    args = eng._insert_rule_args()
    def launch(p):
        _lib.check(eng.lib.infgen_insert_cell_mask(P(eng.pos), P(eng.head), P(eng.state), P(eng.n_agents), P(eng.av), P(k['shape']), S, A, T, c,
                   P(eng.grid_xy), eng.G, args[0], args[1], args[2], args[3], args[4], args[5], args[6], args[7], args[8], P(eng.map_pos),
                   args[9], P(eng.n_map), eng.M_cap, args[10], args[11], args[12], eng.copies, p, P(k['static']), P(k['allowed']), k['W'],
                   P(k['count']), P(k['live']), None, 0, eng.ops.stream), 'infgen_insert_cell_mask')
    for p in (1, 2):
        launch(p); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            launch(p)
        e1.record(); e1.synchronize()
        out['mask_pass%%d_us' %% p] = e0.elapsed_time(e1) * 1e3 / 20
    out['mean_allowed'] = float(k['count'].float().mean().item())
print('RESULT ' + json.dumps(out))
''' % dict(clear=CLEAR, lane=LANE)


def sample(root, variant, scenes, shapes):
    r = subprocess.run([sys.executable, '-c', WORKER, root, variant, str(scenes), shapes], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f'worker {variant} in {root} failed ({r.returncode}):\n{r.stderr[-2000:]}')
    return json.loads(next(line for line in r.stdout.splitlines() if line.startswith('RESULT '))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--scenes', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'insert_rules.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    variants = (['parent'] if a.parent else []) + ['none', 'nothing', 'real']
    got = {v: [] for v in variants}
    lines = [f'# tools/bench_insert_rules.py --scenes {a.scenes} --rounds {a.rounds}' + (' --parent <parent checkout>' if a.parent else '')]
    for rnd in range(a.rounds):
        for v in variants:
            r = sample(a.parent if v == 'parent' else REPO, v, a.scenes, shapes)
            got[v].append(r)
            lines.append(f'sample round={rnd} ' + json.dumps(r))
            print(lines[-1], flush=True)
    med = lambda xs: statistics.median(xs)
    for v in variants:
        ms = [r['rollout_ms'] for r in got[v]]
        lines.append(f'rollout {v}: median {med(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}); inserted rows {got[v][0]["inserted"]}; '
                     f'share within {CLEAR} m of a box {got[v][0]["share_close"]:.4f}; share without a lane token within {LANE} m '
                     f'{got[v][0]["share_no_lane"]:.4f}')
    for p in (1, 2):
        us = [r[f'mask_pass{p}_us'] for r in got['real']]
        lines.append(f'k_insert_cell_mask pass {p} ({"static + clearance" if p == 1 else "clearance only"}): median {med(us):.1f} us per launch '
                     f'(min {min(us):.1f}, max {max(us):.1f}), {a.scenes} scenes')
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-len(variants) - 2:]))


if __name__ == '__main__':
    main()
