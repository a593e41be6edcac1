"""CPU tests of the two slab layouts of convops.py (FlowSlabs, EncLayerSlabs): the pointer arithmetic the stacked decoder /
encoder nodes hand to the native calls, against plain slicing of tensors allocated with the nodes' shapes and dtypes.  No GPU,
no library: the layouts are integers in, integers out."""
import pytest
import torch

from glow_tts_train import convops


def test_encoder_layer_layout_matches_slicing():
    B, H, F_, T, heads, nl = 2, 8, 12, 5, 2, 2
    L = convops.EncLayerSlabs(B, H, F_, T, (heads, 3, 4, 1, -1, 1e-4, 0.1))
    n_ht, n_ft, n_tt = B * H * T, B * F_ * T, B * heads * T * T
    assert L.per == 8 * n_ht + n_ft + n_tt + 4 * B * T and L.wper == 10 * n_ht + n_ft + n_tt
    buf, ws = torch.empty(nl, L.per), torch.empty(nl, L.wper)
    # the independent description: a running cut through the flat buffer in the documented order
    acts = [(n, n_ht, (B, H, T)) for n in ("q", "k", "v", "y_att", "o", "x1", "y2", "x2")]
    acts += [("h", n_ft, (B, F_, T)), ("p_attn", n_tt, (B, heads, T, T)), ("stats1", 2 * B * T, (B, 2, T)), ("stats2", 2 * B * T, (B, 2, T))]
    work = [(n, n_ht, (B, H, T)) for n in ("dx1a", "dy2", "dx1", "dxa", "d_o", "dy_att", "dq", "dk", "dv", "dx")]
    work += [("d_pre", n_ft, (B, F_, T)), ("ds", n_tt, (B, heads, T, T))]
    for slab, floats, parts, table in ((buf, L.per, acts, L.act), (ws, L.wper, work, L.ws)):
        assert sorted(table) == sorted(n for n, _, _ in parts)
        for l in range(nl):
            assert slab[l].data_ptr() - slab.data_ptr() == 4 * l * floats          # how the stack node steps from layer to layer
            off = 0
            for name, n, shape in parts:
                v = slab[l][off: off + n].view(*shape)
                off += n
                assert table[name] == v.data_ptr() - slab[l].data_ptr(), name
                mine = L.view(slab[l], name)
                assert mine.data_ptr() == v.data_ptr() and mine.shape == v.shape and mine.is_contiguous(), name
            assert off == floats
    # the keep-masks: bytes, [attention | branch 1 | FFN | branch 2] per layer
    keep = torch.empty(nl * L.ksz, dtype=torch.uint8)
    off = 0
    for l in range(nl):
        want = []
        for n in (n_tt, n_ht, n_ft, n_ht):
            want.append(keep[off: off + n].data_ptr())
            off += n
        assert list(L.keeps(keep.data_ptr() + l * L.ksz)) == want
    assert off == keep.numel() and L.keeps(None) == (None,) * 4


@pytest.mark.parametrize("first_utt,n_utt", [(0, 4), (2, 2)])
@pytest.mark.parametrize("io", [0, 1, 3])
def test_flow_slab_layout_matches_slicing(io, first_utt, n_utt):
    nb, nl, B, C, H, T, n_split = 3, 2, 4, 8, 16, 6, 4
    fdt = torch.bfloat16 if io & 2 else torch.float32
    adt = torch.bfloat16 if io & 1 else torch.float32
    t = lambda dt, *shape: torch.empty(shape, dtype=dt)                                                   # noqa: E731
    f32 = torch.float32
    x, m2, x_len = t(fdt, B, C, T), t(f32, B, T), t(torch.int32, B)
    drop = t(torch.uint8, nb, nl, B, 2 * H, T)
    z, y, out, y0h = t(fdt, nb, B, C, T), t(fdt, nb, B, C, T), t(f32, nb, B, C, T), t(adt, nb, B, C // 2, T)
    h0, skip = t(adt, nb, B, H, T), t(adt, nb, B, H, T)
    acts, ts, xs = t(adt, nb, nl, B, H, T), t(adt, nb, nl, B, 2 * H, T), t(adt, nb, max(nl - 1, 1), B, H, T)
    logdet, winv = t(f32, nb, B), t(f32, nb, n_split * n_split + 1)
    dz, dlogdet = t(fdt, B, C, T), t(f32, B)
    dy, dx, dout = t(fdt, nb, B, C, T), t(fdt, nb, B, C, T), t(adt, nb, B, C, T)
    dskip, d_xin, dx_wn = t(adt, nb, B, H, T), t(adt, nb, nl, B, 2 * H, T), t(adt, nb, nl, B, H, T)
    p = lambda v: v.data_ptr()                                                                            # noqa: E731
    u = first_utt
    for two_src in (False, True):
        d_rs = t(adt, nb, B, H, T) if two_src else t(adt, nb, nl, B, 2 * H, T)
        L = convops.FlowSlabs(nb, nl, B, C, H, T, io, n_split, 1.25,
                              [p(v) for v in (x, m2, x_len, drop, y, y0h, h0, xs, acts, ts, skip, out, z, logdet, winv)],
                              two_src, [p(v) for v in (dz, dlogdet, dy, dout, dskip, d_rs, d_xin, dx_wn, dx)])
        for k in range(nb):
            lead, pz, pld, w_inv, logdet_w, grads = L.block(k, first_utt, n_utt)
            want = (p((x if k == 0 else z[k - 1])[u:]), p(m2[u:]), p(x_len[u:]), p(drop[k][0, u:]), 1.25, p(y[k][u:]), p(y0h[k][u:]),
                    p(h0[k][u:]), p(xs[k][0, u:]), p(acts[k][0, u:]), p(ts[k][0, u:]), p(skip[k][u:]), p(out[k][u:]))
            assert lead == want, (k, [i for i in range(13) if lead[i] != want[i]])
            assert (lead[L.LEAD_Y], lead[L.LEAD_H0], lead[L.LEAD_SKIP], lead[L.LEAD_OUT]) == (want[5], want[7], want[11], want[12])
            assert (pz, pld, w_inv, logdet_w) == (p(z[k][u:]), p(logdet[k][u:]), p(winv[k]), p(winv[k][n_split * n_split:]))
            want_g = (p((dz if k == nb - 1 else dx[k + 1])[u:]), p(dlogdet[u:]), p(dy[k][u:]), p(dout[k][u:]), p(dskip[k][u:]),
                      p(d_rs[k][u:]) if two_src else p(d_rs[k][0, u:]), p(d_xin[k][0, u:]), p(dx_wn[k][0, u:]), p(dx[k][u:]))
            assert grads == want_g, (k, two_src, [i for i in range(9) if grads[i] != want_g[i]])
    # the forward has no gradient slabs; a slab that is not there yields no pointer; one WN layer keeps no x_{l+1}
    ptrs = [p(v) for v in (x, m2, x_len, drop, y, y0h, h0, xs, acts, ts, skip, out, z, logdet, winv)]
    assert convops.FlowSlabs(nb, nl, B, C, H, T, io, n_split, 1.0, ptrs).block(1, first_utt, n_utt)[5] is None
    ptrs[3] = ptrs[5] = None
    lead = convops.FlowSlabs(nb, 1, B, C, H, T, io, n_split, 1.0, ptrs).block(1, first_utt, n_utt)[0]
    assert lead[3] is None and lead[6] is None and lead[8] is None


def test_flow_slab_layout_refuses_what_lies_outside():
    L = convops.FlowSlabs(2, 2, 4, 8, 16, 6, 0, 4, 1.0, [1 << 20] * 15)
    for bad in ((2, 0, 4), (-1, 0, 4), (0, 2, 3), (0, -1, 2), (1, 4, 1)):
        with pytest.raises(ValueError):
            L.block(*bad)
