"""Restatements for the snapshot tests ("snapshots" of include/infgen_hip.h): the layout of a snapshot entry, the bytes
an entry holds for a context given as flat byte arrays, and the slots / index a save / restore applies after the contract's checks.
Not a test module."""
import numpy as np

D = 128                      # the model width (floats per row of X and of a ring slot)
SCENE_ARRAYS = ('pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag')


def align16(n):
    return (n + 15) // 16 * 16


def segments(A_cap, T, ring, layers, R, token_size, t, logits=True, token_logprob=True, sample_logprob=True, score_steps=0):
    """[(name, kind, bytes of a block, blocks per scene)] in entry order.  kind: 'scene' (one block per scene, scene-major buffer),
    'ring' (`ring` blocks: buffer [ring][S][block]) or 'step' (t blocks: buffer [steps][S][block]).  A segment without blocks
    (a log at t == 0, an absent buffer) takes no room and is not listed."""
    TA = T * A_cap
    out = [('pos', 'scene', TA * 8, 1)] + [(k, 'scene', TA * 4, 1) for k in ('head', 'state', 'token', 'grid')]
    out += [(k, 'scene', TA, 1) for k in ('tmask', 'imask', 'catflag')]
    out.append(('bos', 'scene', A_cap * 4, 1))
    for l in range(layers):
        out += [(('ringK', l), 'ring', A_cap * D * 4, ring), (('ringV', l), 'ring', A_cap * D * 4, ring)]
    out.append(('X', 'scene', A_cap * D * 4, 1))
    out += [('pred_traj', 'scene', A_cap * R * 8, 1), ('pred_head', 'scene', A_cap * R * 4, 1), ('pred_state', 'scene', A_cap * R * 4, 1)]
    if t > 0:
        if token_logprob:
            out.append(('token_logprob', 'step', A_cap * 4, t))
        if sample_logprob:
            out.append(('sample_logprob', 'step', A_cap * 4, t))
        if logits:
            out.append(('logits', 'step', A_cap * token_size * 4, t))
    if score_steps:
        out.append(('step_score', 'scene', score_steps * 8 * 4, 1))
    return out


def entry_bytes(*args, **kw):
    """the bytes of one entry: every block on a 16-byte boundary"""
    return sum(align16(b) * outer for _, _, b, outer in segments(*args, **kw))


def entry(bufs, segs, S, slot):
    """the bytes of slot `slot`'s entry from the context's buffers (name -> flat uint8 numpy array), padding written as 0"""
    parts = []
    for name, kind, b, outer in segs:
        buf = bufs[name]
        for o in range(outer):
            blk = buf.reshape(S, b)[slot] if kind == 'scene' else buf.reshape(-1, S, b)[o, slot]
            parts.append(blk)
            if align16(b) != b:
                parts.append(np.zeros(align16(b) - b, np.uint8))
    return np.concatenate(parts)


def apply_entry(bufs, segs, S, slot, ent):
    """the inverse: entry bytes into slot `slot` of the buffers, in place"""
    off = 0
    for name, kind, b, outer in segs:
        buf = bufs[name]
        for o in range(outer):
            dst = buf.reshape(S, b) if kind == 'scene' else buf.reshape(-1, S, b)[o]
            dst[slot] = ent[off:off + b]
            off += align16(b)
    return off


def head_rows(slots, S, group, t):
    """head [n][4] = slot, group, t, valid of a save, and the number of slots out of range"""
    rows, bad = [], 0
    for s in slots:
        ok = 0 <= s < S
        bad += not ok
        rows.append([s, (group[s] if group is not None else s) if ok else -1, t, int(ok)])
    return np.asarray(rows, np.int64).reshape(-1, 4), bad


def effective_index(index, head, S, group, t):
    """the index a restore applies: an entry out of range, not valid, of another step or of another copy group reads as -1 and is
    counted"""
    idx, bad = [], 0
    n = len(head)
    for s in range(S):
        e = int(index[s])
        if e == -1:
            idx.append(-1)
            continue
        ok = 0 <= e < n
        if ok:
            h = head[e]
            ok = h[3] != 0 and h[2] == t and h[1] == (group[s] if group is not None else s)
        bad += not ok
        idx.append(e if ok else -1)
    return idx, bad
