"""Timing of the rule-based controller (``idm_command``, k_idm_command); bench.py is untouched.

    python tools/bench_idm.py [--parent DIR] [--rounds 3] [--log profiles/idm_command.log]

All on 1024 C3 scenes (64 agents, 1024 map tokens).  Every sample is a fresh process; the variants of a figure alternate
A B A B ... and medians are reported with their spreads.  Figures:

    (a) kernel      one ``infgen_idm_command`` launch - all 65536 rows of the final column controlled, every type on, each row on a
                    route of 8 waypoints laid along its own heading - between device events, against the same poses from torch ops on
                    the same device tensors: explicit differences [S, A, A], the projection of every pair onto the 7 segments
                    [S, A, A, 7], masked arg-mins, gathers and the law.  Inside one process the two alternate; peak device memory of
                    each; the share of rows whose lead agrees and the largest pose difference on those.
    (b) session     an ego-controlled session over all decode steps driven by ``command_idm`` (routes from the log) against the same
                    session driven by pose commands computed beforehand, ``command(poses=...)``.  Both run in THIS tree - the parent has
                    no controller to record the poses with; its session code and decode launches are this tree's - and the figure is
                    device time between events: host work hidden behind a GPU-bound step does not show.
    (c) unchanged   the greedy ``bench.py --gpus 1`` line in this tree against ``--parent`` (a built checkout of the parent commit):
                    a rollout that never calls the controller launches what the parent launches.  Skipped without ``--parent``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, sys
root, mode, warmup, reps, shapes_json = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import constraints, controllers, engine, synth, torch_ops
dev = torch.device('cuda:0')
with open(shapes_json) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
S0, P = 1024, 8
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(S0)]
steps, hc = cfg.num_decode_steps, cfg.hist_columns
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid)
S, A = eng.S, eng.A_cap
med = lambda x: float(np.median(x))
par = controllers.check_idm(dict(types=(1, 1, 1)))

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

def peak(fn):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    r = fn(); torch.cuda.synchronize()
    return r, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

def restated(c, rec, total):
    """the IDM commands of column c from torch ops (all records live) -> pose [S, A, 3], lead [S, A]"""
    p, h, q = eng.pos[:, c], eng.head[:, c], eng.pos[:, c - 1]
    live = (eng.state[:, c] != 0) & (torch.arange(A, device=dev)[None] < eng.n_agents[:, None])
    was = eng.state[:, c - 1] != 0
    ci, si = torch.cos(h)[..., None], torch.sin(h)[..., None]
    inf = torch.tensor(float('inf'), device=dev)
    rot = lambda x, y, c_, s_: (x * c_ + y * s_, y * c_ - x * s_)
    q0x, q0y = rot(rec[..., 0] - p[..., None, 0], rec[..., 1] - p[..., None, 1], ci, si)              # [S, A, M]
    ux, uy = rot(rec[..., 2], rec[..., 3], ci, si)
    L, cum = rec[..., 4], rec[..., 5]
    def project(ex, ey, k):                                                     # points [S, A, (J)] on the row's segments (dim k)
        un = lambda t: t.unsqueeze(2) if k == 3 else t
        rx, ry = ex.unsqueeze(-1) - un(q0x), ey.unsqueeze(-1) - un(q0y)
        t = torch.minimum(torch.clamp(rx * un(ux) + ry * un(uy), min=0.0), un(L))
        fx, fy = rx - t * un(ux), ry - t * un(uy)
        d2, g = (fx * fx + fy * fy).min(-1)
        pick = lambda z: torch.gather(z, -1, g.unsqueeze(-1)).squeeze(-1)
        return pick(un(cum).expand_as(t) + t), d2, g, pick(fx), pick(fy)
    zero = torch.zeros(S, A, device=dev)
    s0, _, g0, fx, fy = project(zero, zero, 2)
    take = lambda z, g: torch.gather(z, -1, g.unsqueeze(-1)).squeeze(-1)
    e0 = fx * -take(uy, g0) + fy * take(ux, g0)
    dv = p - q
    v = torch.where(was, torch.sqrt(dv[..., 0] * dv[..., 0] + dv[..., 1] * dv[..., 1]) / par['dt'], zero)
    d = p[:, None] - p[:, :, None]                                              # [S, A(i), A(j), 2] = pos[j] - pos[i]
    ex, ey = rot(d[..., 0], d[..., 1], ci, si)
    sj, d2, gj, _, _ = project(ex, ey, 3)
    shp = eng._shape10
    thr = par['lateral'] + 0.5 * (shp[:, :, None, 1] + shp[:, None, :, 1])
    ok = live[:, None] & ~torch.eye(A, dtype=torch.bool, device=dev)[None] & (torch.sqrt(d2) <= thr) & (sj > s0[..., None])
    gaps = torch.where(ok, (sj - s0[..., None]) - 0.5 * (shp[:, :, None, 0] + shp[:, None, :, 0]), inf)
    gap, lead = gaps.min(-1)
    vjx, vjy = rot(dv[:, None, :, 0], dv[:, None, :, 1], ci, si)
    gl = take(gj, lead)
    vl = torch.clamp((take(vjx.expand(-1, A, -1), lead) * take(ux, gl) + take(vjy.expand(-1, A, -1), lead) * take(uy, gl)) / par['dt'], min=0.0)
    vl = torch.where(take(was[:, None].expand(-1, A, -1), lead) & torch.isfinite(gap), vl, zero)
    lead = torch.where(torch.isfinite(gap), lead, torch.full_like(lead, -1))
    end = (total - s0) - 0.5 * shp[..., 0]
    at_end = end < gap
    gap, vl, lead = torch.where(at_end, end, gap), torch.where(at_end, zero, vl), torch.where(at_end, torch.full_like(lead, -2), lead)
    v0 = torch.tensor(par['v0'], device=dev)[eng.atype.long().clamp(0, 2)]
    sstar = par['s_min'] + torch.clamp(v * par['headway'] + v * (v - vl) / (2.0 * (par['a_max'] * par['b_comf']) ** 0.5), min=0.0)
    r = v / v0
    qq = sstar / torch.clamp(gap, min=0.1)
    acc = torch.clamp(par['a_max'] * ((1.0 - (r * r) * (r * r)) - qq * qq), -par['b_max'], par['a_max'])
    v1 = torch.clamp(v + acc * par['dt'], min=0.0)
    s1 = torch.minimum(s0 + 0.5 * (v + v1) * par['dt'], total)
    at = torch.clamp((s1[..., None] > cum + L).sum(-1), max=rec.shape[2] - 1)
    a1 = torch.minimum(torch.clamp(s1 - take(cum, at), min=0.0), take(L, at))
    ke = par['keep'] * e0
    tx = (take(q0x, at) + a1 * take(ux, at)) + ke * -take(uy, at)
    tz = (take(q0y, at) + a1 * take(uy, at)) + ke * take(ux, at)
    c1, s1_ = ci[..., 0], si[..., 0]
    pose = torch.stack([p[..., 0] + (tx * c1 - tz * s1_), p[..., 1] + (tx * s1_ + tz * c1), torch.atan2(take(rec[..., 3], at), take(rec[..., 2], at))], -1)
    return pose, lead

out = dict(rows=int(eng.rows), slots=S, steps=steps)
if mode == 'kernel':
    eng.rollout()
    c = hc + steps - 1
    # every row on a route of P waypoints along its own heading, bending by 0.05 rad per 15 m segment, from 20 m behind it
    k = torch.arange(P, device=dev, dtype=torch.float32)
    ang = eng.head[:, c, :, None] + 0.05 * torch.cumsum(torch.cat([k[:1] * 0, k[1:] * 0 + 1.0]), 0)[None, None]
    seg = 15.0 * torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    start = eng.pos[:, c] - 20.0 * torch.stack([torch.cos(eng.head[:, c]), torch.sin(eng.head[:, c])], -1)
    routes = (start[:, :, None] + torch.cumsum(seg, 2) - seg[:, :, :1]).contiguous()
    rec, total = torch_ops.route_records(routes, torch.full((S, A), P, dtype=torch.int32, device=dev))
    ctl = torch.ones(S, A, dtype=torch.uint8, device=dev)
    res = controllers.idm_buffers(S, A, dev)
    pose = torch.zeros(S, A, 3, device=dev)
    kernel = lambda: controllers.launch(eng.lib, eng.ops.stream, eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, eng._shape10, ctl, c,
                                        rec, total, 1, None, par, pose, res)
    _, kpeak = peak(kernel)
    want, tpeak = peak(lambda: restated(c, rec, total))
    ruled = res['state'].view(S, A, 8)[..., 7] == 1
    same = (res['lead'].view(S, A) == want[1]) & ruled
    err = float((pose - want[0]).abs()[same].max())
    share = float(same.sum()) / float(ruled.sum())
    del want
    for _ in range(warmup):
        kernel(); restated(c, rec, total)
    torch.cuda.synchronize()
    ka, ta = [], []
    for _ in range(reps):
        ka.append(timed(kernel)); ta.append(timed(lambda: restated(c, rec, total)))
    out.update(ms=med(ka), all_ms=ka, torch_ms=med(ta), torch_all_ms=ta, kernel_peak_mib=kpeak, torch_peak_mib=tpeak,
               ruled_rows=int(ruled.sum()), rows_with_equal_lead=share, max_abs_pose_diff_on_those=err,
               rows_with_a_lead=float((res['lead'] >= 0).float().mean()))
else:                                  # 'session_poses' / 'session_idm'
    routes, n = constraints.routes_from_logged(scenes, start=hc - 1)
    def session(record=None):
        ses = eng.session(controlled='ego', pose='token')
        while not ses.done:
            if mode == 'session_idm' or record is not None:
                ses.command_idm(routes=routes, n_points=n)
                if record is not None:
                    record.append(ses._pose.clone())
            else:
                ses.command(poses=plan[ses.t])
            ses.advance()
    plan = []
    session(plan)                      # the poses the controller commands, for the variant that is handed them
    for _ in range(warmup):
        session()
    torch.cuda.synchronize()
    ms = [timed(session) for _ in range(reps)]
    out.update(ms=med(ms), all_ms=ms, per_step_ms=med(ms) / steps)
print(json.dumps(out))
'''


def run(cmd, **kw):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, **kw)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'{cmd[1:4]} failed ({out.returncode}): {out.stderr[-1500:]}')
    return json.loads(lines[-1])


def bench_line(root, steps, warmup):
    line = run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                '--no-cpu-baseline', '--no-parity', '--no-literal', '--no-strict', '--no-balance'], cwd=root)
    return dict(ms=line['value'], unit=line.get('unit'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (figure c)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=15)
    ap.add_argument('--bench-steps', type=int, default=3)
    ap.add_argument('--figures', default='abc')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'idm_command.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    worker = lambda mode, reps=a.reps: run([sys.executable, '-c', WORKER, REPO, mode, str(a.warmup), str(reps), shapes])
    figures = []
    if 'a' in a.figures:
        figures.append(('(a) one idm_command launch against torch ops, 65536 controlled rows, routes of 8 waypoints (ms)',
                        [('kernel', lambda: worker('kernel', a.kernel_reps))]))
    if 'b' in a.figures:
        figures.append(('(b) ego-controlled session of 1024 scenes: command_idm per step against pose commands computed beforehand (ms per session)',
                        [('poses', lambda: worker('session_poses')), ('idm', lambda: worker('session_idm'))]))
    if 'c' in a.figures and a.parent:
        parent = os.path.abspath(a.parent)
        figures.append((f'(c) greedy bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.warmup} line (its own unit)',
                        [('parent', lambda: bench_line(parent, a.bench_steps, a.warmup)), ('this', lambda: bench_line(REPO, a.bench_steps, a.warmup))]))
    results = []

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, 'w') as f:
            f.write('\n'.join(json.dumps(r) for r in results) + '\n')

    for figure, variants in figures:
        entry = dict(figure=figure, rounds=0)
        results.append(entry)
        got = {name: [] for name, _ in variants}
        for r in range(a.rounds):
            for name, fn in variants:          # alternating: one sample of every variant per round
                s = fn()
                got[name].append(s)
                ms = [x['ms'] for x in got[name]]
                entry[name] = dict(median=statistics.median(ms), min=min(ms), max=max(ms), samples=ms)
                entry[name].update({k: v for k, v in s.items() if k not in ('ms', 'all_ms', 'torch_ms', 'torch_all_ms')})
                if name == 'kernel':
                    tm = [x['torch_ms'] for x in got[name]]
                    entry[name].update(torch_median=statistics.median(tm), torch_min=min(tm), torch_max=max(tm), torch_samples=tm,
                                       torch_over_kernel=statistics.median(tm) / statistics.median(ms))
                print(f'{figure}: round {r} {name}: {s["ms"]:.4f}', flush=True)
                write()
            entry['rounds'] = r + 1
        if 'parent' in entry:
            entry['this_median_inside_parents_spread'] = entry['parent']['min'] <= entry['this']['median'] <= entry['parent']['max']
        if 'idm' in entry:
            add = entry['idm']['median'] - entry['poses']['median']
            entry.update(added_ms_per_session=add, added_us_per_step=1e3 * add / entry['idm']['steps'])
        write()
        print(json.dumps(entry), flush=True)


if __name__ == '__main__':
    main()
