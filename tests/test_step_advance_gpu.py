"""Operator-level tests of the step-advance kernels: k_integrate through infgen_integrate, the raw-feature gather (k_rawfeat_prep /
rawfeat_prep_item) through infgen_raw_feature and infgen_raw_feature_rows, on hand-built blocks against tests/graph_ref.py.  States,
tokens, grid cells and masks are compared exactly, poses within graph_ref.BAR_STEP_* and the motion pair within BAR_MOTION_* (four
times the error of an fp32 numpy evaluation against float64); everything a call must leave alone is compared bitwise, and every
array a kernel could write carries a guard tail.  The Fourier embedding and the fusion MLP behind the gather are judged in
test_ops_gpu.py / test_precision_gpu.py: here only their wiring is checked, bitwise against the same entries called by the test."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import graph_ref as gr
from gpu_blocks import SENT_F, dev, device_block, guard_intact, lib_and_check

pytestmark = pytest.mark.gpu

STATE_KEYS = ('pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'type', 'bos', 'pred_traj', 'pred_head',
              'pred_state')
INPUT_KEYS = ('next_token', 'next_state', 'teacher_token', 'teacher_state', 'teacher_grid', 'teacher_pos', 'teacher_head', 'replay_row')
SCRATCH_KEYS = ('raw2', 'cat', 'fus_in', 'tmp1', 'tmp2', 'X')


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def merged(st, ext, **more):
    blk = dict(st)
    blk.update({k: v for k, v in ext.items() if v is not None})
    blk.update(more)
    return blk


def host(blk, ten, keys):
    """the arrays `keys` of the block after a call, their guard tails checked"""
    torch.cuda.synchronize()
    got = {}
    for k in keys:
        n = blk[k].size
        assert guard_intact(ten[k], n), f'{k}: written beyond its end'
        got[k] = ten[k][:n].cpu().numpy().reshape(blk[k].shape)
    return got


# ------------------------------------------------------------------------------------------------ integrate
def run_integrate(st, ext, t):
    lib, check = lib_and_check()
    blk = merged(st, ext)
    keys = [k for k in STATE_KEYS + INPUT_KEYS if isinstance(blk.get(k), np.ndarray)]
    b, ten = device_block(blk, guard=keys)
    check(lib.infgen_integrate(C.byref(b), t, None), 'infgen_integrate')
    return host(blk, ten, keys)


@pytest.mark.parametrize('name', list(gr.INTEGRATE_CASES))
def test_integrate(name):
    """every graph_ref.INTEGRATE_CASES entry (2 / 64 / 1 workgroups per scene; the ego in its own, the first, the last or another
    workgroup; n_agents 0, 1, 16, 17, A_cap; grids of 1 .. 2049 cells in LDS and in global memory; the state rules; teacher arrays
    with and without replay_row; exact ties).  state, token, grid, imask, catflag and pred_state of the WHOLE block equal the
    reference's exactly, so columns other than n and rows >= n_agents are untouched; pos, head, pred_traj, pred_head are bitwise
    their inputs outside column n / the step's five slots of the live rows and within the bars inside; tmask, type, bos and every
    input array stay (the reference's line 2230 clears another mask than the one the temporal edges read)."""
    st, ext, t = gr.gen_integrate(name)
    ref = gr.integrate_ref(st, ext, t)
    got = run_integrate(st, ext, t)
    S, A_cap, T, R = st['S'], st['A_cap'], st['T'], st['R']
    n, sl = 2 + t, slice(t * 5, t * 5 + 5)
    live = np.arange(A_cap)[None] < st['n_agents'][:, None]
    for k in ('state', 'token', 'grid', 'imask', 'catflag'):
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (k, [(tuple(i), int(got[k][tuple(i)]), int(ref[k][tuple(i)])) for i in bad[:8]])
    assert np.array_equal(got['pred_state'].astype(np.float64), ref['pred_state'])
    blk = merged(st, ext)
    for k in ('tmask', 'type', 'bos') + INPUT_KEYS:
        if k in got:
            assert same(got[k], blk[k]), k
    m = np.zeros((S, T, A_cap), bool)
    m[:, n] = live
    pm = np.zeros((S * A_cap, R), bool)
    pm[:, sl] = live.reshape(-1)[:, None]
    for k, mask in (('pos', m), ('head', m), ('pred_traj', pm), ('pred_head', pm)):
        assert np.array_equal(bits(got[k])[~mask], bits(st[k])[~mask]), f'{k}: written outside the step'
    inv = m & (ref['state'] == gr.INVALID)
    assert (got['pos'][inv] == 0).all() and (got['head'][inv] == 0).all()
    e = gr.step_errors(ref, got, st, t)
    print(f'integrate {name}: device errors position {e[0]:.3g} m (bar {gr.BAR_STEP_POS:.3g}) heading {e[1]:.3g} rad '
          f'(bar {gr.BAR_STEP_HEAD:.3g}); {int(live.sum())} rows, {int(inv.sum())} of them INVALID')
    assert e[0] <= gr.BAR_STEP_POS and e[1] <= gr.BAR_STEP_HEAD


@pytest.mark.parametrize('name', ['replay_ego', 'ties', 'g2_last'])
def test_integrate_same_scene_in_both_splits(name):
    """the scenes of an S = 3 batch (2 workgroups per scene, the ego integrated again by the workgroup that does not own it) repeated
    through an S = 129 batch (1 workgroup per scene): every array bitwise the same scene by scene"""
    st, ext, t = gr.gen_integrate(name)
    few = run_integrate(st, ext, t)
    scenes = [i % st['S'] for i in range(129)]
    st2, ext2 = gr.take_step_scenes(st, ext, scenes)
    assert gr.integrate_groups(st['S'], st['A_cap']) == 2 and gr.integrate_groups(st2['S'], st2['A_cap']) == 1
    many = run_integrate(st2, ext2, t)
    want, _ = gr.take_step_scenes(dict(few, S=st['S'], A_cap=st['A_cap']), {}, scenes)
    for k in STATE_KEYS:
        assert same(many[k], want[k]), k


def test_integrate_replay_flags_all_and_none():
    """replay_row all 1 is bitwise replay_row = NULL (the teacher arrays apply to every row); all 0 is bitwise the run without any
    teacher array"""
    st, ext, t = gr.gen_integrate('replay_ego')
    flags = ext['replay_row']
    assert 0 < flags.sum() < flags.size
    ones, null = run_integrate(st, dict(ext, replay_row=np.ones_like(flags)), t), run_integrate(st, dict(ext, replay_row=None), t)
    zeros = run_integrate(st, dict(ext, replay_row=np.zeros_like(flags)), t)
    plain = run_integrate(st, dict(ext, **{k: None for k in INPUT_KEYS[2:]}), t)
    mixed = run_integrate(st, ext, t)
    for k in STATE_KEYS:
        assert same(ones[k], null[k]), k
        assert same(zeros[k], plain[k]), k
    assert not same(mixed['pos'], null['pos']) and not same(mixed['pos'], plain['pos'])


# ------------------------------------------------------------------------------------------------ raw feature
@functools.lru_cache(maxsize=None)
def packs():
    """x_a_emb (Fourier, 2 inputs + categorical) and fusion_emb with 512 and with 384 inputs (no grid embedding) of seeded weights"""
    from conftest import make_weights
    from infgen_amd import packing
    sd = make_weights()
    w0 = 'agent_encoder.fusion_emb.mlp.0.weight'
    return (packing.pack_fourier(sd, 'agent_encoder.x_a_emb', 2), packing.pack_mlp_embedding(sd, 'agent_encoder.fusion_emb'),
            packing.pack_mlp_embedding(dict(sd, **{w0: np.ascontiguousarray(sd[w0][:, :384])}), 'agent_encoder.fusion_emb'))


def rawfeat_block(st, ext, no_grid):
    four, fus512, fus384 = packs()
    blk = merged(st, ext, four_xa=four, fusion_pack=fus384 if no_grid else fus512, no_grid_token=no_grid)
    b, ten = device_block(blk, guard=SCRATCH_KEYS)
    return blk, b, ten


def check_gather(got, ref, n, no_grid):
    """slots [0, n) of raw2 / cat / fus_in against the reference's rows, slots >= n untouched"""
    f32 = np.float32
    raw2, cat, fus = got['raw2'], got['cat'], got['fus_in']
    for k in ('raw2', 'cat', 'fus_in'):
        assert (got[k][n:] == f32(SENT_F)).all(), f'{k}: written beyond slot {n}'
    assert same(cat[:n], ref['cat'].astype(f32)) and same(fus[:n, 0:128], ref['tok'].astype(f32))
    assert same(fus[:n, 256:384], ref['state'].astype(f32))
    if no_grid:
        assert (fus[:n, 384:512] == f32(SENT_F)).all()
    else:
        assert same(fus[:n, 384:512], ref['grid'].astype(f32))
    assert (raw2[:n, 2:] == 0).all()
    assert (raw2[:n, 0][ref['ruled'] == 1] == f32(np.sqrt(2.0))).all() and (raw2[:n, 0][ref['ruled'] == 2] == f32(2 * np.sqrt(2.0))).all()
    en = np.abs(raw2[:n, 0].astype(np.float64) - ref['raw2'][:, 0]).max()
    eb = gr.ang_err(raw2[:n, 1], ref['raw2'][:, 1]).max()
    assert en <= gr.BAR_MOTION_NORM and eb <= gr.BAR_MOTION_BEARING, (en, eb)
    return en, eb


def wiring(ten, blk, n):
    """-> (x_a embedding, fusion output) of the first n slots: infgen_fourier_embed / infgen_mlp_embedding called with the arguments
    the raw-feature entries pass, on the device's own raw2 / cat and fus_in"""
    lib, check = lib_and_check()
    xa = torch.full((n, 512), SENT_F, device=dev())
    check(lib.infgen_fourier_embed(ten['raw2'].data_ptr(), 2, None, n, ten['four_xa'].data_ptr(), ten['cat'].data_ptr(), 128,
                                   xa.data_ptr() + 128 * 4, 512, 0, None), 'infgen_fourier_embed')
    y, t1, t2 = (torch.full((n, 128), SENT_F, device=dev()) for _ in range(3))
    check(lib.infgen_mlp_embedding(ten['fus_in'].data_ptr(), 512, n, 384 if blk['no_grid_token'] else 512, ten['fusion_pack'].data_ptr(),
                                   t1.data_ptr(), t2.data_ptr(), y.data_ptr(), 128, None), 'infgen_mlp_embedding')
    torch.cuda.synchronize()
    return xa.cpu().numpy()[:, 128:256], y.cpu().numpy()


@pytest.mark.parametrize('col,no_grid', [(0, 0), (1, 0), (2, 0), (1, 1)])
def test_raw_feature(col, no_grid):
    """columns 0 (the enter rule), 1 and 2 of graph_ref.gen_rawfeat: previous INVALID / current valid, previous valid / current
    INVALID, both INVALID, tokens -1 / -2, grid -1, catflag 0 / 1, the three types.  The gathered rows bitwise, the motion pair within
    the bars with the gap rules' norms exactly float32(sqrt 2) / float32(2 sqrt 2); with no_grid_token columns 384.. of fus_in keep
    their sentinel; fus_in[:, 128:256] and X bitwise what the two embedding entries give on the device's own inputs"""
    lib, check = lib_and_check()
    st, ext = gr.gen_rawfeat()
    rows = st['S'] * st['A_cap']
    blk, b, ten = rawfeat_block(st, ext, no_grid)
    check(lib.infgen_raw_feature(C.byref(b), col, None), 'infgen_raw_feature')
    got = host(blk, ten, SCRATCH_KEYS)
    ref = gr.rawfeat_prep_ref(st, dict(ext, no_grid_token=no_grid), col)
    en, eb = check_gather(got, ref, rows, no_grid)
    print(f'raw feature col {col}: device errors motion norm {en:.3g} m (bar {gr.BAR_MOTION_NORM:.3g}) bearing {eb:.3g} rad '
          f'(bar {gr.BAR_MOTION_BEARING:.3g})')
    xa, y = wiring(ten, blk, rows)
    assert same(got['fus_in'][:, 128:256], xa) and same(got['X'], y)
    assert np.isfinite(got['X']).all() and np.abs(got['X']).max() < 1e6
    for k in STATE_KEYS:
        assert same(ten[k].cpu().numpy(), st[k]), k


@contextlib.contextmanager
def attn_mode(mode):
    """the process-wide attn_mode for the calls inside (0: fusion_emb as three fp32 k_linear launches through tmp1 / tmp2)"""
    lib, check = lib_and_check()
    check(lib.infgen_set_attn_mode(mode), 'infgen_set_attn_mode')
    try:
        yield
    finally:
        check(lib.infgen_set_attn_mode(2), 'infgen_set_attn_mode')


@pytest.mark.parametrize('n,mode', [pytest.param(1, 2, id='1'), pytest.param(33, 2, id='33'), pytest.param(96, 2, id='96'),
                                    pytest.param(1, 0, id='1-fp32'), pytest.param(33, 0, id='33-fp32'), pytest.param(96, 0, id='96-fp32')])
def test_raw_feature_rows(n, mode):
    """a shuffled row_list with a mask that has holes, n = 1, 33 and S * A_cap: compact slots (a masked-off slot gathers row 0), X
    written at the listed unmasked rows only - bitwise the fusion of the compact fus_in - and untouched everywhere else.  attn_mode 2
    (the default: k_mlpemb_h) and 0, where the entry's fusion writes tmp1, tmp2 and tmp1 again (its output aliases the first stage's)
    and must still equal infgen_mlp_embedding with three separate arrays"""
    with attn_mode(mode):
        _raw_feature_rows(n)


def _raw_feature_rows(n):
    lib, check = lib_and_check()
    st, ext = gr.gen_rawfeat()
    rows, col = st['S'] * st['A_cap'], 2
    assert n <= rows and (n < 34 or n == rows)
    rng = np.random.default_rng(n)
    row_list = rng.permutation(rows)[:n].astype(np.int32)
    mask = (rng.uniform(size=n) > 0.3).astype(np.int32)
    mask[0], mask[1 % n] = 1, (0 if n > 1 else 1)
    blk, b, ten = rawfeat_block(st, ext, 0)
    dl, dm = torch.from_numpy(row_list).to(dev()), torch.from_numpy(mask).to(dev())
    check(lib.infgen_raw_feature_rows(C.addressof(b), col, dl.data_ptr(), dm.data_ptr(), n, None), 'infgen_raw_feature_rows')
    got = host(blk, ten, SCRATCH_KEYS)
    check_gather(got, gr.rawfeat_prep_ref(st, ext, col, rows=row_list, mask=mask), n, 0)
    xa, y = wiring(ten, blk, n)
    assert same(got['fus_in'][:n, 128:256], xa)
    on = mask != 0
    assert same(got['X'][row_list[on]], y[on])
    rest = np.ones(rows, bool)
    rest[row_list[on]] = False
    assert (got['X'][rest] == np.float32(SENT_F)).all() and rest.sum() == rows - on.sum() and (n == 1 or (~on).any())


def test_raw_feature_rows_refuses_more_rows_than_the_layout():
    """n = S * A_cap + 1: a non-zero return with its text and no launch; n = 0: 0 and no launch"""
    from infgen_amd import _lib
    lib = _lib.load()
    st, ext = gr.gen_rawfeat()
    rows = st['S'] * st['A_cap']
    blk, b, ten = rawfeat_block(st, ext, 0)
    dl, dm = torch.zeros(rows + 1, dtype=torch.int32, device=dev()), torch.ones(rows + 1, dtype=torch.int32, device=dev())
    assert lib.infgen_raw_feature_rows(C.addressof(b), 1, dl.data_ptr(), dm.data_ptr(), rows + 1, None) != 0
    assert 'more rows than the layout holds' in lib.infgen_last_error().decode()
    assert lib.infgen_raw_feature_rows(C.addressof(b), 1, dl.data_ptr(), dm.data_ptr(), 0, None) == 0
    got = host(blk, ten, SCRATCH_KEYS)
    for k in SCRATCH_KEYS:
        assert (got[k] == np.float32(SENT_F)).all(), k
