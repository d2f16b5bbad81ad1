"""Many-row attention, forward and backward, on every mask geometry, against float64.

Every kernel of the family derives from (x_len or x_len_dev[b], kv_len[b], q_off, block origin) whether a tile is skipped,
taken without the element mask, or masked element by element — attn_rows_kernel per 128-query block and 32-key tile, the fused
backward per key chunk / 32-query tile / 32-key wave, attn_dq_reduce_kernel per slab, the two-kernel backward with queries and
then keys as lanes, attn16_kernel over 64-key tiles.  The cases (tests/oracle_runners.py, ATTN_GEOMETRY_CASES) put x_len,
kv_len and T on the remainders 0, 1 and -1 of each block size; the reference is the visibility rule of include/valle_hip.h
written out element by element in float64.  tests/test_attn_geometry_cpu.py shows that reference to be torch autograd's, the
cases to reach the edges, and ten planted geometry faults to miss by more than 10 x these tolerances.

Tolerances: out atol 3e-5 (test_kernels_gpu.test_attn_rows), dq / dk / dv atol 6e-5 + rtol 1e-4 (test_train_gpu.
test_attn_rows_bwd_vs_torch_autograd), the 16-bit forward those of test_bf16_gpu.test_attn_rows_bf16.  lse2 — the row's
log-sum-exp in base 2, added up tile by tile with the hardware exp2 / log2 — may be off by SUM_MARGIN = 4 times the error the
same quantity has when plain fp32 torch computes it on the CPU: ATTN_FP32_ERR holds that measurement per case and quantity
(plus 20 % for a CPU whose BLAS adds in another order, rounded up to two digits; the CPU file asserts it still holds).  The
figures come from the reference's arithmetic, never from a kernel."""
import functools

import pytest
import torch

from tests import oracle_runners as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# the fp32 emulation's worst error against float64 (R.attn_geometry_reference at float32), per case and quantity
ATTN_FP32_ERR = {
    'prefix_small': {'out': 8.7e-07, 'lse2': 9.4e-07, 'dq': 1.7e-06, 'dk': 5.3e-06, 'dv': 5.7e-06},
    'prefix_mid': {'out': 1.2e-06, 'lse2': 1.4e-06, 'dq': 1.1e-06, 'dk': 2e-06, 'dv': 2.3e-06},
    'prefix_long': {'out': 9.3e-07, 'lse2': 1.5e-06, 'dq': 9.1e-07, 'dk': 1.6e-06, 'dv': 1.4e-06},
    'prefix_512': {'out': 1.1e-06, 'lse2': 1.4e-06, 'dq': 9.5e-07, 'dk': 1.6e-06, 'dv': 2.1e-06},
    'prefix_scalar': {'out': 6e-07, 'lse2': 1.4e-06, 'dq': 5.7e-07, 'dk': 8.5e-07, 'dv': 9.4e-07},
    'full_small': {'out': 1.1e-06, 'lse2': 1.1e-06, 'dq': 2.4e-06, 'dk': 4.6e-06, 'dv': 6.8e-06},
    'full_mid': {'out': 8.5e-07, 'lse2': 1.2e-06, 'dq': 1.2e-06, 'dk': 2e-06, 'dv': 9.8e-07},
    'full_long': {'out': 1.1e-06, 'lse2': 1.4e-06, 'dq': 1.5e-06, 'dk': 2.7e-06, 'dv': 4e-06},
    'full_512': {'out': 6.2e-07, 'lse2': 1.4e-06, 'dq': 4.9e-07, 'dk': 7e-07, 'dv': 5.1e-07},
    'explicit_shared': {'out': 1.2e-06, 'lse2': 1.4e-06, 'dq': 1.4e-06, 'dk': 9.4e-07, 'dv': 9.4e-07},
    'explicit_bmask': {'out': 7.9e-07, 'lse2': 1.1e-06},
    'prefix_tq_lt_tk': {'out': 4.9e-07, 'lse2': 1.4e-06},
    'full_tq_lt_tk': {'out': 5.7e-07, 'lse2': 1.3e-06},
    'empty_row_full': {'out': 1.3e-06, 'lse2': 1.5e-06, 'dq': 9.8e-07, 'dk': 1.1e-06, 'dv': 1e-06},
    'empty_row_prefix': {'out': 6.7e-07, 'lse2': 1.4e-06, 'dq': 8.5e-07, 'dk': 1.2e-06, 'dv': 1.3e-06},
    'empty_row_small': {'out': 8.1e-07, 'lse2': 1.1e-06, 'dq': 8.2e-07, 'dk': 1.4e-06, 'dv': 1.5e-06},
}
BWD_CASES = [n for n, c in R.ATTN_GEOMETRY_CASES.items() if c[2] == c[3]]
ANALYTIC_CASES = [n for n, c in R.ATTN_GEOMETRY_CASES.items() if c[4] != 'explicit']
KNOB_ATTN_BWD, KNOB_ATTN_BWD_CHUNKS = 13, 14            # VH_TUNE_ATTN_BWD, VH_TUNE_ATTN_BWD_CHUNKS (include/valle_hip.h)
PAD_COLS = 8                                            # columns of the out / dout buffers beyond d (ldo = d + 8)


@functools.lru_cache(maxsize=None)
def reference(name, h16=None):
    """The float64 reference of a case, computed once and shared (nobody writes into it)."""
    return R.attn_geometry_reference(name, h16=h16)


def rows(t):
    """(B, h, T, 64) -> (B * T, h * 64): heads in columns, as the kernels read q and write out."""
    B, h, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, h * 64)


def heads(t, B, h):
    """(B * T, h * 64) -> (B, h, T, 64) on the CPU."""
    return t.detach().cpu().reshape(B, -1, h, 64).permute(0, 2, 1, 3)


def cache(t, S_max, beyond, dtype=torch.float32):
    """K or V in the cache layout (B, h, S_max, 64) with `beyond` in the rows from Tk on: they must never be read."""
    B, h, Tk, _ = t.shape
    c = torch.full((B, h, S_max, 64), beyond, dtype=dtype)
    c[:, :, :Tk] = t
    return c.to(DEV)


def device_spec(K, mode, spec):
    kw = dict(mode={'full': K.MASK_FULL, 'prefix': K.MASK_PREFIX, 'explicit': K.MASK_EXPLICIT}[mode])
    kw.update({k: (v if isinstance(v, int) else v.to(DEV)) for k, v in spec.items()})
    return kw


class Forward:
    """A case on the device and its fp32 forward.  q is read in place from a (B * Tq, 3 d) buffer whose other columns are
    NaN; out goes into the first d columns of a NaN-filled (B * Tq, d + 8) buffer; the caches hold S_max = Tk + 9 rows, NaN (K)
    and Inf (V) from Tk on, finite randn in [kv_len, Tk) (the kernel multiplies those by p = 0)."""

    def __init__(self, name, operands=None):
        from valle2_amd import kernels as K
        self.K, self.name = K, name
        self.B, self.h, self.Tq, self.Tk, mode = R.ATTN_GEOMETRY_CASES[name]
        q, k, v, dout, _, spec = R.attn_geometry_inputs(name)
        if operands is not None:                       # (q, k, v, dout) in place of the case's own (tests/attn_scores.py)
            q, k, v, dout = operands
        self.d = d = 64 * self.h
        qkv = torch.full((self.B * self.Tq, 3 * d), float('nan'))
        qkv[:, :d] = rows(q)
        self.q = qkv.to(DEV)[:, :d]
        dbuf = torch.full((self.B * self.Tq, d + PAD_COLS), float('nan'))
        dbuf[:, :d] = rows(dout)
        self.dout = dbuf.to(DEV)[:, :d]
        self.kc, self.vc = cache(k, self.Tk + 9, float('nan')), cache(v, self.Tk + 9, float('inf'))
        self.spec = device_spec(K, mode, spec)
        self.per_row_mask = mode == 'explicit' and spec['mask'].dim() == 3

    def run(self, with_lse2):
        obuf = torch.full((self.B * self.Tq, self.d + PAD_COLS), float('nan'), device=DEV)
        lse2 = torch.full((self.B, self.h, self.Tq), float('nan'), device=DEV) if with_lse2 else None
        self.K.attn_rows(self.q, self.kc, self.vc, obuf[:, :self.d], self.B, self.h, self.Tq, self.Tk, lse2=lse2, **self.spec)
        assert bool(torch.isnan(obuf[:, self.d:]).all()), 'columns beyond d were written'
        return obuf[:, :self.d], lse2


@pytest.mark.parametrize('name', list(R.ATTN_GEOMETRY_CASES))
def test_forward_fp32(name):
    """attn_rows_kernel: kmax / n_tiles per 128-query block, any / all per wave and 32-key tile, the element mask."""
    f = Forward(name)
    ref = reference(name)
    plain, _ = f.run(False)
    got = dict(out=heads(plain, f.B, f.h))
    if not f.per_row_mask:                         # (a per-row mask is inference only: vh_attn_rows_bmask writes no lse2)
        out, lse2 = f.run(True)
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), 'out differs between the runs with and without lse2'
        got['lse2'] = lse2.cpu()
    kept = R.attn_kept_rows(name)
    for qn, g_ in got.items():
        print(f'{name} {qn}: worst error {R.worst(g_[kept], ref[qn][kept]):.3e}')
    R.check_attn(name, got, ref, ATTN_FP32_ERR[name]['lse2'])


def backward_forms(f):
    """(label, VH_TUNE_ATTN_BWD, VH_TUNE_ATTN_BWD_CHUNKS) to run: the default form with the model's chunk count, with the
    fewest chunks and with two larger counts (a forced count that collapses onto one already run is skipped), the two-kernel
    form."""
    from valle2_amd import _lib
    L = _lib.lib()
    nc_min = -(-f.Tk // 256)
    forms, seen = [], set()
    for forced in (0, 1, nc_min + 1, 2 * nc_min + 2):
        L.vh_set_tuning(KNOB_ATTN_BWD_CHUNKS, forced)
        try:
            nc = L.vh_attn_rows_bwd_chunks(f.B, f.h, f.Tk, f.spec['mode'])
        finally:
            L.vh_set_tuning(KNOB_ATTN_BWD_CHUNKS, 0)
        if forced == 1:
            assert nc == nc_min, (nc, nc_min)
        if nc not in seen:
            seen.add(nc)
            forms.append((f'fused-{nc}-chunks-of-{R.attn_chunk_keys(f.Tk, nc)}', 0, forced))
    return forms + [('two-kernel', 1, 0)]


@pytest.mark.parametrize('name', BWD_CASES)
def test_backward(name):
    """attn_bwd_fused_kernel<4> / <8> + attn_dq_reduce_kernel at every chunk plan, attn_bwd_dq_kernel + attn_bwd_dkv_kernel:
    dq, dk, dv from the forward's own out / lse2 (NaN / -inf in a row without a key) into the three column blocks of one
    NaN-filled (B * T, 3 d) buffer; a second run is bit-identical; a row without a key gets exact zeros."""
    from valle2_amd import _lib
    L = _lib.lib()
    f = Forward(name)
    ref = reference(name)
    out, lse2 = f.run(True)
    d, failed = f.d, []
    for label, form, forced in backward_forms(f):
        L.vh_set_tuning(KNOB_ATTN_BWD, form)
        L.vh_set_tuning(KNOB_ATTN_BWD_CHUNKS, forced)
        try:
            runs = []
            for _ in range(2):
                g_ = torch.full((f.B * f.Tk, 3 * d), float('nan'), device=DEV)
                f.K.attn_rows_bwd(f.q, f.kc, f.vc, out, f.dout, lse2, g_[:, :d], g_[:, d:2 * d], g_[:, 2 * d:], f.B, f.h, f.Tk,
                                  **f.spec)
                runs.append(g_)
        finally:
            L.vh_set_tuning(KNOB_ATTN_BWD, 0)
            L.vh_set_tuning(KNOB_ATTN_BWD_CHUNKS, 0)
        got = {qn: heads(runs[0][:, i * d:(i + 1) * d], f.B, f.h) for i, qn in enumerate(('dq', 'dk', 'dv'))}
        print(f'{name} {label}: ' + ', '.join(f'{qn} {R.worst(got[qn], ref[qn]):.3e}' for qn in got))
        try:
            assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), 'a second run differs'
            R.check_attn(name, got, ref, None)
        except AssertionError as e:
            failed.append(f'{label}: {e}')
    assert not failed, ' || '.join(failed)


@pytest.mark.parametrize('name', ANALYTIC_CASES)
def test_forward_16bit(name):
    """attn16_kernel (klim, kend, wave_kend, need_mask over 64-key tiles): operands narrowed to the build's 16-bit format,
    q pre-scaled as vh_linear_qkv_bf16 leaves it, against float64 attention over the same rounded operands with the
    tolerances of test_bf16_gpu.test_attn_rows_bf16."""
    from valle2_amd import kernels as K
    from valle2_amd._lib import h16_dtype
    H16 = h16_dtype()
    fp16 = H16 == torch.float16
    B, h, Tq, Tk, mode = R.ATTN_GEOMETRY_CASES[name]
    q, k, v, _, _, spec = R.attn_geometry_inputs(name)
    assert K.Q16_PRESCALE == R.ATTN_Q16_PRESCALE
    d = 64 * h
    qbuf = torch.full((B * Tq, 3 * d), float('nan'), dtype=H16)
    qbuf[:, :d] = (rows(q) * K.Q16_PRESCALE).to(H16)
    obuf = torch.full((B * Tq, d + PAD_COLS), float('nan'), dtype=H16, device=DEV)
    K.attn_rows_bf16(qbuf.to(DEV)[:, :d], cache(k.to(H16), Tk + 9, float('nan'), H16), cache(v.to(H16), Tk + 9, float('inf'), H16),
                     obuf[:, :d], B, h, Tq, Tk, **device_spec(K, mode, spec))
    assert bool(torch.isnan(obuf[:, d:]).all()), 'columns beyond d were written'
    kept = R.attn_kept_rows(name)
    got, ref = heads(obuf[:, :d], B, h).double()[kept], reference(name, H16)['out'][kept]
    print(f'{name}: worst error {R.worst(got, ref):.3e}')
    torch.testing.assert_close(got, ref, atol=1e-3 if fp16 else 6e-3, rtol=2 * (2 ** -10 if fp16 else 2 ** -8))
