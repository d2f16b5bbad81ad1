"""Many-row flash attention at head widths other than 64 (`vh_attn_rows_hd`, kernels.attn_rows_hd).

The kernel is checked against float64 torch on the CPU computed from the SAME strided views — q / k / v the per-head column
blocks of one (B T, 3 h hd) buffer, out those of a (B T, h hd) buffer — at every NB = ceil(hd / 32) instantiation, at query
counts on both sides of the 32-key tile and the 128-query block, under every analytic mask form; the buffers' unused columns
and the output buffer are NaN before the call.  Tolerance: test_kernels_gpu.py::test_attn_rows' own (atol 3e-5, rtol 2e-5);
measured worst error over all cases of a width: 0.8e-6 (hd 16) to 1.7e-6 (hd 96).  Width 64 is cross-checked against
`vh_attn_rows` on the same data, a row with kv_len = 0 included.  The stack does not call the kernel yet."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ATOL, RTOL = 3e-5, 2e-5
B, H = 2, 3
GAP = 4                       # NaN columns after the last head of every buffer row
# 31 / 32 / 33: the key tile; 127 / 128 / 129: the query block; 200: two blocks, the second partial; 1: a single query
TS = [1, 31, 32, 33, 127, 128, 129, 200]


def g(seed):
    return torch.Generator().manual_seed(seed)


def _buffers(hd, Tq, Tk, seed):
    """(qkv, out) on the CPU: qkv (B Tk, 3 H hd) and out (B Tq, H hd) as the leading columns of buffers GAP columns wider,
    the gap NaN, out NaN all over."""
    ld, ldo = 3 * H * hd + GAP, H * hd + GAP
    big = torch.full((B * Tk, ld), float('nan'))
    big[:, :3 * H * hd] = torch.randn(B * Tk, 3 * H * hd, generator=g(seed))
    outb = torch.full((B * Tq, ldo), float('nan'))
    return big, outb


def _views(big, outb, hd, Tq, Tk):
    """The (B, H, T, hd) views of q (the last Tq rows of every batch row), k, v and out inside the two buffers."""
    ld, ldo = big.stride(0), outb.stride(0)
    qkv = big.as_strided((B, Tk, 3, H, hd), (Tk * ld, ld, H * hd, hd, 1))
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    out = outb.as_strided((B, Tq, H, hd), (Tq * ldo, ldo, hd, 1)).permute(0, 2, 1, 3)
    return q[:, :, Tk - Tq:], k, v, out


def _visible(Tq, Tk, mode, xl, kvl):
    """(B, Tq, Tk) bool, the header's semantics: query i sits at key position Tk - Tq + i."""
    j = torch.arange(Tk)[None, None, :]
    p = (Tk - Tq + torch.arange(Tq))[None, :, None]
    kv = torch.as_tensor(kvl).view(-1, 1, 1).expand(B, 1, 1)
    vis = (j < kv).expand(B, Tq, Tk)
    if mode == 'prefix':
        x = torch.as_tensor(xl).view(-1, 1, 1)
        vis = vis & ((j < x) | ((p >= x) & (j <= p)))
    return vis


def _ref64(q, k, v, vis):
    s = (q.double() @ k.double().transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    s = s.masked_fill(~vis[:, None], float('-inf'))
    return torch.softmax(s, dim=-1) @ v.double()


def _mask_cases(T):
    kvl = (T, max(1, T - 37))
    return [('full', 'full', 0, None, None), ('full+kv_len', 'full', 0, None, kvl), ('causal', 'prefix', 0, None, None),
            ('prefix1', 'prefix', 1, None, None), ('prefix33', 'prefix', 33, None, None), ('prefixT', 'prefix', T, None, None),
            ('prefix_dev+kv_len', 'prefix', 0, (min(5, T), min(40, T)), kvl)]


def _run(K, big_d, outb_d, hd, Tq, Tk, mode, xl, xl_dev, kvl):
    q, k, v, out = _views(big_d, outb_d, hd, Tq, Tk)
    dev = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32, device=DEV)
    K.attn_rows_hd(q, k, v, out, hd ** -0.5, mode=K.MASK_PREFIX if mode == 'prefix' else K.MASK_FULL, x_len=xl,
                   x_len_dev=dev(xl_dev), kv_len=dev(kvl))


def _check(K, hd, Tq, Tk, name, mode, xl, xl_dev, kvl, seed, worst):
    big, outb = _buffers(hd, Tq, Tk, seed)
    q, k, v, _ = _views(big, outb, hd, Tq, Tk)
    vis = _visible(Tq, Tk, mode, xl if xl_dev is None else xl_dev, kvl if kvl is not None else (Tk, Tk))
    ref = _ref64(q, k, v, vis)                                   # (B, H, Tq, hd)
    big_d, outb_d = big.to(DEV), outb.to(DEV)
    _run(K, big_d, outb_d, hd, Tq, Tk, mode, xl, xl_dev, kvl)
    got_buf = outb_d.cpu()
    assert torch.equal(big_d.cpu().isnan(), big.isnan()), 'the q / k / v buffer was written'
    assert got_buf[:, H * hd:].isnan().all(), f'hd={hd} T={Tq} {name}: columns outside the h*hd outputs were written'
    got = got_buf[:, :H * hd].view(B, Tq, H, hd).permute(0, 2, 1, 3)
    assert not got.isnan().any(), f'hd={hd} Tq={Tq} Tk={Tk} {name}: NaN in the output'
    err = (got.double() - ref).abs().max().item()
    worst[0] = max(worst[0], err)
    print(f'attn_rows_hd hd={hd} Tq={Tq} Tk={Tk} {name}: max|err| vs float64 = {err:.3e}')
    torch.testing.assert_close(got, ref.float(), atol=ATOL, rtol=RTOL, msg=lambda m: f'hd={hd} Tq={Tq} Tk={Tk} {name}: {m}')


@pytest.mark.parametrize('hd', [16, 20, 32, 48, 64, 96, 100, 128])
def test_kernel_matches_float64_on_strided_views(hd):
    from valle2_amd import kernels as K
    worst = [0.0]
    for T in TS:
        for i, (name, mode, xl, xl_dev, kvl) in enumerate(_mask_cases(T)):
            _check(K, hd, T, T, name, mode, xl, xl_dev, kvl, 1000 * hd + 10 * T + i, worst)
    _check(K, hd, 5, 70, 'Tq<Tk prefix33', 'prefix', 33, None, None, 1000 * hd + 7, worst)
    print(f'attn_rows_hd hd={hd}: worst max|err| = {worst[0]:.3e}')


@pytest.mark.parametrize('mode', ['full', 'prefix'])
def test_width_64_agrees_with_vh_attn_rows_including_an_empty_row(mode):
    """Mask semantics against the existing width-64 kernel on the same data; batch row 0 has kv_len = 0: NaN rows in both."""
    from valle2_amd import kernels as K
    hd, T, xl = 64, 150, 41
    big, outb = _buffers(hd, T, T, 64)
    big_d, outb_d = big.to(DEV), outb.to(DEV)
    kvl = (0, T - 3)
    _run(K, big_d, outb_d, hd, T, T, mode, xl, None, kvl)
    got = outb_d[:, :H * hd].view(B, T, H * hd)
    q, k, v, _ = _views(big_d, outb_d, hd, T, T)
    ref = torch.empty(B * T, H * hd, device=DEV)
    K.attn_rows(q.permute(0, 2, 1, 3).reshape(B * T, H * hd).contiguous(), k.contiguous(), v.contiguous(), ref, B, H, T, T,
                K.MASK_PREFIX if mode == 'prefix' else K.MASK_FULL, x_len=xl, kv_len=torch.tensor(kvl, dtype=torch.int32, device=DEV))
    ref = ref.view(B, T, H * hd)
    assert got[0].isnan().all() and ref[0].isnan().all()
    assert not got[1].isnan().any()
    torch.testing.assert_close(got[1].cpu(), ref[1].cpu(), atol=ATOL, rtol=RTOL)
    assert outb_d[:, H * hd:].isnan().all()


def test_python_wrapper_refuses_what_the_kernel_does_not_take():
    from valle2_amd import _lib, kernels as K
    x = torch.zeros(2, 3, 8, 32, device=DEV)
    with pytest.raises(_lib.VhError, match='caller-supplied masks'):
        K.attn_rows_hd(x, x, x, x.clone(), 1.0, mode=K.MASK_EXPLICIT, mask=torch.zeros(8, 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.VhError, match='unit stride'):
        K.attn_rows_hd(x.transpose(2, 3), x.transpose(2, 3), x.transpose(2, 3), x.transpose(2, 3).clone(), 1.0, mode=K.MASK_FULL)
    with pytest.raises(_lib.VhError, match='head_dim=200'):
        y = torch.zeros(1, 1, 8, 200, device=DEV)
        K.attn_rows_hd(y, y, y, y.clone(), 1.0, mode=K.MASK_FULL)
