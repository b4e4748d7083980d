"""Device-side helpers shared by the operator-level GPU tests (test_edge_builders_gpu.py, test_insertion_ops_gpu.py,
test_step_advance_gpu.py, test_forward_ops_gpu.py): guarded device buffers, InfgenEdgeBuf (whole, or the upper zone of a buffer
that several edge sets share) / InfgenRollout blocks over device copies of a graph_ref block.  What the tests assert of an edge
buffer's contents is graph_ref.compare_lists.  Not a test module and not a conftest; torch and the library are only needed by
the callers, which are GPU tests."""
import numpy as np
import torch

GUARD = 64
SENT_I, SENT_F, SENT_B = -123456789, -7.25e30, 0xA5


def dev():
    return torch.device('cuda:0')


def guarded(n, dtype, width=1):
    """a device buffer of n (x width) elements plus a guard tail of GUARD (x width), all filled with a sentinel"""
    t = torch.empty((n + GUARD) * width, device=dev(), dtype=dtype)
    t.fill_(SENT_F if dtype == torch.float32 else SENT_I)
    return t


def _sentinel(dtype):
    return SENT_F if dtype == torch.float32 else SENT_B if dtype == torch.uint8 else SENT_I


def guard_intact(t, n, width=1):
    tail = t[n * width:]
    return bool((tail == _sentinel(t.dtype)).all())


def guarded_copy(v):
    """a flat device copy of a numpy array (float32, int32 or uint8) followed by a guard tail of GUARD sentinels"""
    flat = torch.from_numpy(np.ascontiguousarray(v).reshape(-1))
    t = torch.empty(flat.numel() + GUARD, device=dev(), dtype=flat.dtype)
    t.fill_(_sentinel(flat.dtype))
    t[:flat.numel()] = flat.to(dev())
    return t


class Edges:
    """an InfgenEdgeBuf of `rows` destinations and `cap` edges, every array guarded.  base > 0: the zone [base, base + cap) of a
    src / raw buffer of base + cap edges, as the forward shares one buffer between two edge sets (off entries then carry the base)"""

    def __init__(self, rows, cap, base=0):
        from infgen_amd import _lib
        self.rows, self.cap, self.base = rows, cap, base
        self.off, self.cnt = guarded(rows, torch.int32), guarded(rows, torch.int32)
        self.src, self.raw = guarded(base + cap, torch.int32), guarded(base + cap, torch.float32, 4)
        self.total = guarded(1, torch.int32)
        self.buf = _lib.EdgeBuf()
        self.buf.off, self.buf.cnt = self.off.data_ptr(), self.cnt.data_ptr()
        self.buf.src, self.buf.raw = self.src.data_ptr() + 4 * base, self.raw.data_ptr() + 16 * base
        self.buf.total, self.buf.cap = self.total.data_ptr(), cap

    def host(self):
        """-> (off, cnt, src, raw, total): src / raw of the whole buffer, the zone's base included"""
        torch.cuda.synchronize()
        n = self.base + self.cap
        assert guard_intact(self.off, self.rows) and guard_intact(self.cnt, self.rows) and guard_intact(self.total, 1)
        assert guard_intact(self.src, n) and guard_intact(self.raw, n, 4), 'written at or beyond cap'
        return (self.off[:self.rows].cpu().numpy(), self.cnt[:self.rows].cpu().numpy(), self.src[:n].cpu().numpy(),
                self.raw[:4 * n].cpu().numpy().reshape(-1, 4), int(self.total[0].item()))


STEP_POINTERS = ('next_token', 'next_state', 'teacher_token', 'teacher_state', 'teacher_grid', 'teacher_pos', 'teacher_head',
                 'replay_row', 'vocab', 'tok_tab', 'grid_tab', 'state_emb', 'cat_agent', 'cat_seed', 'raw2', 'cat', 'fus_in', 'tmp1',
                 'tmp2', 'X', 'four_xa', 'fusion_pack')
STEP_SCALARS = ('force_valid', 'no_state_token', 'no_grid_token')


def device_block(st, edges=None, guard=()):
    """InfgenRollout over device copies of a graph_ref block (and, when the dict holds them, of what graph_ref.new_step_ext adds:
    absent or None keys stay null / zero); the arrays named in `guard` are flat copies with a guard tail (guarded_copy).
    -> (block, the tensors by name)"""
    from infgen_amd import _lib
    ten = {}
    for k, v in st.items():
        if isinstance(v, np.ndarray):
            ten[k] = guarded_copy(v) if k in guard else torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    b = _lib.Rollout()
    b.S, b.A_cap, b.T, b.M_cap, b.W, b.ring, b.R = st['S'], st['A_cap'], st['T'], st['M_cap'], st['W'], st['ring'], st['R']
    b.token_size, b.grid_size, b.num_layers = 2048, st['grid_size'], 1
    b.r_map, b.r_agent = st['r_map'], st['r_agent']
    for k in ('n_agents', 'n_map', 'av_index', 'pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'type', 'bos',
              'map_pos', 'map_orient', 'map_scene', 'first_new', 'hv_ovr', 'grid_xy', 'pred_traj', 'pred_head', 'pred_state'):
        if k in ten:
            setattr(b, k, ten[k].data_ptr())
    for k in STEP_POINTERS:
        if k in ten:
            setattr(b, k, ten[k].data_ptr())
    for k in STEP_SCALARS:
        if st.get(k) is not None:
            setattr(b, k, int(st[k]))
    if edges:
        b.et, b.em, b.ea = edges['t'].buf, edges['m'].buf, edges['a'].buf
    return b, ten


def lib_and_check():
    from infgen_amd import _lib
    return _lib.load(), _lib.check
