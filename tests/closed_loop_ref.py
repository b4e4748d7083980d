"""NumPy float64 restatement of the closed-loop command kernel's matching rule (k_command_rows) and the synthetic
cases the CPU and GPU tests share.  Inputs are the float32 values the kernel reads; everything after that is float64."""
import numpy as np

INVALID, VALID = 0, 1
S, A_CAP, T = 2, 16, 6
N_AGENTS = (11, 16)
SHAPES = np.asarray([[4.8, 2.0, 1.6], [1.0, 1.0, 1.8], [2.0, 1.0, 1.7]], np.float32)     # (length, width, height) per type
# the margin between two costs the fp32 kernel is asked to tell apart, in units of np.spacing(float32(max |coordinate|)) = eps.
# A world corner of a token: two products and two sums (<= eps / 2 each) plus the cosf / sinf error on token extents (< 9 m) below the
# coordinate magnitude (2 ulp of 1 times the extent: <= eps) -> 3 eps; a corner of the commanded box: <= 2 eps; their difference: 5.5 eps per axis, the
# distance sqrt(2) x that plus its own rounding: <= 9 eps; four corners and three sums: < 40 eps per cost, 80 eps between two
MARGIN_EPS = 80
SEED = 20300            # picked on the CPU: the restatement decides >= 98 % of the matched rows beyond the margin (test_closed_loop_cpu.py)


def box_contour(x, y, head, width, length):
    """the commanded box (token_kernels.hip box_contour): left front, right front, right back, left back -> (4, 2)"""
    x, y, head, width, length = (float(v) for v in (x, y, head, width, length))
    hc, hs = 0.5 * np.cos(head), 0.5 * np.sin(head)
    lc, ls, wc, ws = length * hc, length * hs, width * hc, width * hs
    return np.asarray([[x + lc - ws, y + ls + wc], [x + lc + ws, y + ls - wc], [x - lc + ws, y - ls - wc], [x - lc - ws, y - ls + wc]])


def world_contours(last, pos, head):
    """the last contours ``last`` [n][4][2] of a vocabulary moved by a stored pose, k_integrate's transform -> [n][4][2]"""
    last = np.asarray(last, np.float64)
    cs, sn = np.cos(float(head)), np.sin(float(head))
    wx = last[..., 0] * cs - last[..., 1] * sn + float(pos[0])
    wy = last[..., 0] * sn + last[..., 1] * cs + float(pos[1])
    return np.stack([wx, wy], -1)


def costs(last, pos, head, cmd, width, length):
    """cost of every token: the sum over the four corners of the distance to the commanded box's -> [n]"""
    d = world_contours(last, pos, head) - box_contour(cmd[0], cmd[1], cmd[2], width, length)[None]
    return np.sqrt((d ** 2).sum(-1)).sum(-1)


def match(last, pos, head, cmd, width, length):
    """-> (token: the first minimum, its cost, the gap to the second smallest cost)"""
    c = costs(last, pos, head, cmd, width, length)
    k = int(np.argmin(c))                              # (np.argmin returns the first minimum)
    rest = np.delete(c, k)
    return k, float(c[k]), float(rest.min() - c[k]) if rest.size else np.inf


def integrate(contour, pos, head):
    """the pose k_integrate makes of one token's last contour [4][2] from a stored pose -> (x, y, heading)"""
    w = world_contours(np.asarray(contour)[None], pos, head)[0]
    return w[:, 0].mean(), w[:, 1].mean(), np.arctan2(w[0, 1] - w[3, 1], w[0, 0] - w[3, 0])


def kernel_case(seed, vocab, t=1):
    """one launch's inputs and the restatement's outputs: 2 scenes x A_cap 16, n_agents (11, 16), all three types.  Flagged: row 0,
    the last valid row, a row >= n_agents, a row without a command (mask 0), a row whose stored state is invalid, and about two
    thirds of the rest.  Commands: a random token of the row's type integrated from its stored pose, moved by up to 0.3 m / 0.1 rad.
    Stored positions within +-12 m (the margin scales with the coordinate magnitude, the gaps between neighbouring pedestrian
    tokens do not: at +-60 m a tenth of the rows would sit inside the margin).  ``vocab`` [3][n][6][4][2] float32."""
    rng = np.random.default_rng(seed)
    n_tok = vocab.shape[1]
    c, n = 1 + t, 2 + t
    assert n < T
    atype = rng.integers(0, 3, (S, A_CAP)).astype(np.int32)
    atype[:, :3] = np.arange(3)
    shape = (SHAPES[atype] * rng.uniform(0.9, 1.1, (S, A_CAP, 1))).astype(np.float32)
    pos = rng.uniform(-12, 12, (S, T, A_CAP, 2)).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A_CAP)).astype(np.float32)
    state = np.full((S, T, A_CAP), VALID, np.int32)
    flag = (rng.random((S, A_CAP)) < 0.66)
    mask = np.ones((S, A_CAP), np.uint8)
    flag[:, 0] = True
    flag[0, N_AGENTS[0] - 1] = flag[1, N_AGENTS[1] - 1] = True
    flag[0, 12] = True                                  # >= n_agents: untouched
    flag[1, 3] = True; mask[1, 3] = 0                   # no command: leaves
    flag[1, 7] = True; state[1, c, 7] = INVALID         # already out: stays out
    flag[0, 5] = False; flag[1, 9] = False              # (and rows that are not controlled)
    cmd_tok = rng.integers(0, n_tok, (S, A_CAP)).astype(np.int32)
    cmd_pose = np.zeros((S, A_CAP, 3), np.float32)
    exp_tok = np.full((S, A_CAP), -1, np.int64); exp_state = np.zeros((S, A_CAP), np.int64)
    cost = np.zeros((S, A_CAP)); gap = np.full((S, A_CAP), np.inf); matched = np.zeros((S, A_CAP), bool)
    written = np.zeros((S, A_CAP), bool)
    for s in range(S):
        for r in range(A_CAP):
            last = vocab[atype[s, r], :, 5]
            x, y, h = integrate(last[cmd_tok[s, r]], pos[s, c, r], head[s, c, r])
            ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.3)
            cmd_pose[s, r] = (x + rad * np.cos(ang), y + rad * np.sin(ang), h + rng.uniform(-0.1, 0.1))
            if not flag[s, r] or r >= N_AGENTS[s]:
                continue
            written[s, r] = True
            if state[s, c, r] == INVALID or mask[s, r] == 0:
                continue
            exp_state[s, r] = VALID
            matched[s, r] = True
            exp_tok[s, r], cost[s, r], gap[s, r] = match(last, pos[s, c, r], head[s, c, r], cmd_pose[s, r], shape[s, r, 1], shape[s, r, 0])
    coord = max(float(np.abs(pos).max()), float(np.abs(cmd_pose[..., :2]).max())) + float(shape.max())
    margin = MARGIN_EPS * float(np.spacing(np.float32(coord)))
    return dict(t=t, c=c, n=n, n_agents=np.asarray(N_AGENTS, np.int32), atype=atype, shape=shape, pos=pos, head=head, state=state,
                flag=flag.astype(np.uint8), mask=mask, cmd_tok=cmd_tok, cmd_pose=cmd_pose, exp_tok=exp_tok, exp_state=exp_state,
                cost=cost, gap=gap, matched=matched, written=written, margin=margin)


def vocabularies():
    """the full synthetic vocabulary and one whose size (1000) is no multiple of the kernel's 256 threads -> [3][n][6][4][2] each"""
    from infgen_amd import synth
    return [np.stack([v[k] for k in ('veh', 'ped', 'cyc')]).astype(np.float32)
            for v in (synth.make_agent_vocab(2048), synth.make_agent_vocab(1000))]


def kernel_cases():
    """the launches of the kernel test: four draws per vocabulary, decode steps 0 .. 3"""
    return [(v, kernel_case(SEED + 10 * i + j, v, t=j)) for i, v in enumerate(vocabularies()) for j in range(4)]


def decided_share(cases):
    g = np.concatenate([k['gap'][k['matched']] for _, k in cases])
    m = np.concatenate([np.full(int(k['matched'].sum()), k['margin']) for _, k in cases])
    return float((g > m).mean()), int(g.size)
