"""occlusion(), lesion() and integrated_gradients() between 71 and 416 nodes (csrc/occlusion.hip, csrc/lesion.hip,
csrc/saliency.hip + csrc/intgrad.hip over csrc/gnm_rowblock.h) against the fp64 oracle, on the case table of
tests/rowblock_midrange_cases.py: n in {97, 129, 190, 256, 257, 401, 416} x H in {32, 64, 128} x m in {1, 2, 3}, L = 3,
every pooling form, an undirected and a directed graph per case, sparse and dense.  What the shapes reach (the second
half-row word group away from n = 400, the wrapped request ring of rb_bits_product at every H and tail, dead rows behind
12 full blocks, kRbMaxN, the transposed bits above 70 nodes, a second finish launch for more than 8 classes) is stated
and checked in tests/test_rowblock_midrange_host.py, with the conditions on the references the bounds here rest on.

Bounds.  lesion() and occlusion(): helpers.Calibrated, max(RTOL, 4 x err) with err the distance of the independent fp32
CPU forward (TorchCpuGIN) from the fp64 oracle ON THE SAME DELETED COPIES -- at most 2e-5 by the host test's cap, never a
HIP output; max-norm relative to the graph's max |base|, NaN patterns equal.  All n columns of occlusion() are checked
against the kernel's formulation in fp64 on the source graph (masked_forward64_sets, pinned to the oracle on explicit
copies at 1e-12 by the host test), the named columns against the oracle on explicit copies.  integrated_gradients(): the
flat RTOL = 1e-5 relative to the graph's max |attr|.

MEASURED on an MI355X (pytest -s prints them; also in DESIGN.md sections 3.12 - 3.14), worst error per n = 97, 129,
190, 256, 257, 401, 416 (bound 1e-5 unless stated):
  lesion()                 6.0e-7  7.0e-7  4.7e-7  7.0e-7  2.3e-6 (bound 1.18e-5: H = 32, m = 2, average / sum, no learned
                           eps, where the fp32 CPU forward is 3.0e-6 from fp64)  6.4e-7  5.4e-7
  occlusion()              6.7e-7  7.1e-7  6.0e-7  9.5e-7  2.3e-6 (the same case; the one-hot case 2.25e-6)  6.4e-7  6.1e-7
  lesion() on one-node sets against occlusion(): at most 1.6e-6 (the one-hot case at n = 257)
  integrated_gradients()   6.7e-7  6.2e-7  8.4e-7  7.1e-7  5.4e-7  5.1e-7  5.6e-7; no case declined
  the ragged batch 2.4e-7; 11 classes 4.6e-7 (n = 129) and 4.6e-7 (n = 257); the chunked calls (5 and 3 launches of the
  entries) and every batch size bitwise.
With the default seed the case n = 256, H = 128, m = 3 (sum / average, no learned eps, K = 1) gave 5.3e-3 for
integrated_gradients(): one pre-activation at 1.5e-8 of its layer's largest, a ReLU mask fp32 does not determine -- the
reason for rowblock_midrange_cases.IG_RELU_MARGIN, a condition on the fp64 oracle alone, and for the seeds it replaced.
"""
import numpy as np
import pytest
import torch

import rowblock_midrange_cases as T
import test_gpu_lesion as LES
import test_gpu_occlusion as OCC
from helpers import RTOL, Calibrated, rel_err
from test_gpu_intgrad import worst_err
from test_gpu_occlusion import state64
from test_gpu_saliency import POOLS, model_of

pytestmark = pytest.mark.gpu


def model_for(case):
    """model_of's model of a case, which must be the one the CPU references were computed for"""
    a, kw = T.model_args(case)
    model = model_of(*a, **kw)
    got, want = state64(model), T.state_of(case)
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want), case.id
    return model


def noise_of(base32, base64, les32, les64):
    """a Calibrated that has seen the fp32 CPU forward's distance on this graph's base and finite copies"""
    cal = Calibrated()
    cal.noise = T.fp32_noise(base32, base64, les32, les64)
    return cal, max(cal.base, cal.factor * cal.noise)


def check_lesion(got, d, base64, base32, les64, les32, want_nan, classes=None):
    """graph d of test_gpu_lesion.run()'s result against its references; returns (worst error, bound)"""
    cl = list(range(base64.shape[0])) if classes is None else list(classes)
    cal = Calibrated()
    scale = float(np.abs(base64).max())
    cal.check(got[1][:, d], base32[cl], base64[cl], "base", floor=scale)
    cal.check(got[2][d], les32[:, cl], les64[:, cl], "lesioned", floor=scale)
    nan = np.isnan(got[2][d])
    assert (nan.any(1) == want_nan).all() and (nan.all(1) == want_nan).all()
    return max(e for _, e, _, _ in cal.log), cal.log[-1][3]


def check_occlusion(got, d, base64, bound, occ, classes=None):
    """graph d of test_gpu_occlusion.run()'s result: base, all n columns against masked_forward64_sets, the named
    columns against the oracle on explicit copies"""
    cl = list(range(base64.shape[0])) if classes is None else list(classes)
    scale = float(np.abs(base64).max())
    e0 = rel_err(got[1][:, d], base64[cl], floor=scale)
    e1 = T.err(got[2][d], occ.masked64[:, cl], scale)
    e2 = T.err(got[2][d][occ.named], occ.named64[:, cl], scale)
    assert T.err(occ.masked64[occ.named], occ.named64, scale) <= 1e-12         # (the pin of the host test, on this array)
    assert max(e0, e1, e2) <= bound, "base %.3e all columns %.3e named columns %.3e > %.2e" % (e0, e1, e2, bound)
    return max(e0, e1, e2)


def test_the_table_is_built_on_this_files_pooling_forms():
    assert T.POOLS == POOLS


# ---------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("n", T.NODES)
def test_lesion(n):
    worst = bound = 0.0
    for case in T.cases(n):
        model, gs, refs = model_for(case), T.graphs_of(case), T.lesion_reference(case)
        got = LES.run(model, gs, [r.sets for r in refs], batch_size=3)             # (delta = base - lesioned bitwise)
        for d, r in enumerate(refs):
            e, b = check_lesion(got, d, r.base64, r.base32, r.les64, r.les32, r.want_nan)
            print("  %s graph %d: %.2e (bound %.2e)" % (case.id, d, e, b))
            if e / b > worst / max(bound, 1e-30) or bound == 0.0:
                worst, bound = e, b
    print("lesion n=%d: worst %.2e under %.2e" % (n, worst, bound))


@pytest.mark.parametrize("n", T.NODES)
def test_occlusion(n):
    worst = bound = worst_les = 0.0
    for case in T.cases(n):
        model, gs = model_for(case), T.graphs_of(case)
        lref, oref = T.lesion_reference(case), T.occlusion_reference(case)
        got = OCC.run(model, gs)
        named = oref[0].named
        one = np.eye(n, dtype=bool)[named]
        _, _, les = model.lesion(gs, (0, 1), one, return_scores=True)              # [C, G, k]: the same one-node sets
        for d, (r, occ) in enumerate(zip(lref, oref)):
            _, b = noise_of(r.base32, r.base64, r.les32, r.les64)
            e = check_occlusion(got, d, r.base64, b, occ)
            el = T.err(les[:, d].t().cpu().numpy(), got[2][d][named], float(np.abs(r.base64).max()))
            assert el <= RTOL, "%s graph %d: lesion() on one-node sets is %.3e from occlusion()" % (case.id, d, el)
            print("  %s graph %d: %.2e (bound %.2e), lesion vs occlusion %.2e" % (case.id, d, e, b, el))
            worst_les = max(worst_les, el)
            if e / b > worst / max(bound, 1e-30) or bound == 0.0:
                worst, bound = e, b
    print("occlusion n=%d: worst %.2e under %.2e; lesion() on one-node sets against occlusion() %.2e" %
          (n, worst, bound, worst_les))


@pytest.mark.parametrize("n", T.NODES)
def test_integrated_gradients(n):
    worst, declined = 0.0, 0
    for case in T.cases(n):
        model, gs = model_for(case), T.graphs_of(case)
        kw = dict(steps=case.K, baseline=T.baseline_of(case), method=case.method)
        if any(T.ig_declined(case, g) for g in gs):
            with pytest.raises(ValueError, match="isolated node"):
                model.integrated_gradients(gs, (0, 1), **kw)
            declined += 1
            continue
        attr, base, _, _ = model.integrated_gradients(gs, (0, 1), return_scores=True, **kw)
        assert attr.shape == (2, 2, n, case.F0) and attr.dtype == torch.float32
        e = worst_err(attr, T.ig_reference(case))
        print("  %s K=%d %s baseline=%d: %.2e" % (case.id, case.K, case.method, case.baseline, e))
        assert e <= RTOL, "%s: %.3e > %.1e" % (case.id, e, RTOL)
        assert torch.equal(base, model.predict(gs)[:, [0, 1]].t())
        worst = max(worst, e)
    print("integrated_gradients n=%d: worst %.2e under %.1e, %d cases declined" % (n, worst, RTOL, declined))


# ---------------------------------------------------------------------------------------------- across the word groups
def test_ragged_batch_across_the_word_group_boundary():
    """graphs of 33, 256, 257, 416 and 2 nodes in one lesion() call (1 .. 5 sets each) and one occlusion() call: both
    half-row word-group sizes under one mask stride and one block count; each graph alone gives the same bits"""
    gs, sets, lref, oref = T.ragged_reference()
    model = model_for(T.RAGGED_CASE)
    got = LES.run(model, gs, sets)
    assert isinstance(got[0], list) and [tuple(x.shape) for x in got[0][0]] == [(k,) for k in range(1, 6)]
    occ = OCC.run(model, gs)
    worst = bound = 0.0
    for d, (g, S, (b64, b32, l64, l32, want)) in enumerate(zip(gs, sets, lref)):
        e, b = check_lesion(got, d, b64, b32, l64, l32, want)
        e = max(e, check_occlusion(occ, d, b64, b, oref[d]))
        print("  %d nodes: %.2e (bound %.2e)" % (len(g.g), e, b))
        if e / b > worst / max(bound, 1e-30) or bound == 0.0:
            worst, bound = e, b
        alone = LES.run(model, [g], [S])
        assert np.array_equal(alone[1][:, 0], got[1][:, d]) and np.array_equal(alone[2][0], got[2][d], equal_nan=True)
        alone = OCC.run(model, [g])
        assert np.array_equal(alone[1][:, 0], occ[1][:, d]) and np.array_equal(alone[2][0], occ[2][d], equal_nan=True)
    print("ragged batch: worst %.2e under %.2e" % (worst, bound))


def test_chunks_and_batch_sizes_at_eight_half_row_words(monkeypatch):
    """n = 257, 5 graphs x 6 sets: the scratch budgets lowered until lesion() runs in 5 chunks and occlusion() in 3 --
    bitwise the unchunked result, as is every batch size"""
    from gnm import attribution, core
    from gnm._cabi import lib
    model, gs, sets = model_for(T.CHUNK_CASE), T.chunk_graphs(), T.chunk_sets()
    d0, b0, l0 = model.lesion(gs, (0, 1), sets, return_scores=True)
    e0, c0, o0 = model.occlusion(gs, (0, 1), return_scores=True)
    assert l0.shape == (2, 5, 6) and o0.shape == (2, 5, 257) and torch.isfinite(l0[:, :, 0]).all()
    nn = lambda t: torch.nan_to_num(t, nan=7.0)                                    # noqa: E731
    for bs in (1, 3, 8):
        d, b, o = model.lesion(gs, (0, 1), sets, batch_size=bs, return_scores=True)
        assert torch.equal(nn(d), nn(d0)) and torch.equal(b, b0) and torch.equal(nn(o), nn(l0)), bs
        d, b, o = model.occlusion(gs, (0, 1), batch_size=bs, return_scores=True)
        assert torch.equal(nn(d), nn(e0)) and torch.equal(b, c0) and torch.equal(nn(o), nn(o0)), bs
    calls = {"gnm_lesion": 0, "gnm_occlusion": 0}

    def counted(name):
        real = getattr(lib, name)

        def call(*a):
            calls[name] += 1
            return real(*a)
        return call

    monkeypatch.setattr(core.lib, "gnm_lesion", counted("gnm_lesion"), raising=False)
    monkeypatch.setattr(core.lib, "gnm_occlusion", counted("gnm_occlusion"), raising=False)
    monkeypatch.setattr(attribution, "LESION_SCRATCH_BYTES", 4 * int(lib.gnm_lesion_scratch_floats(7 * 257, 7, 257, 64, 3)))
    monkeypatch.setattr(attribution, "OCCLUSION_SCRATCH_BYTES",
                        4 * int(lib.gnm_occlusion_scratch_floats(2 * 257 * 257, 2 * 257, 257, 64, 3)))
    d, b, o = model.lesion(gs, (0, 1), sets, batch_size=8, return_scores=True)     # 30 virtual graphs, 7 to a chunk
    assert calls["gnm_lesion"] == 5
    assert torch.equal(nn(d), nn(d0)) and torch.equal(b, b0) and torch.equal(nn(o), nn(l0))
    d, b, o = model.occlusion(gs, (0, 1), batch_size=8, return_scores=True)        # 5 graphs, 2 to a chunk
    assert calls["gnm_occlusion"] == 3
    assert torch.equal(nn(d), nn(e0)) and torch.equal(b, c0) and torch.equal(nn(o), nn(o0))
    print("chunks: lesion %d calls, occlusion %d calls, bitwise" % (calls["gnm_lesion"], calls["gnm_occlusion"]))


@pytest.mark.parametrize("case", T.CLASS_CASES, ids=[c.id for c in T.CLASS_CASES])
def test_more_than_eight_classes(case):
    """11 classes, asked for as a shuffled 10-tuple and as all 11: both finish kernels run a second launch that writes
    at out + 8 ldo.  Per class against the fp64 oracle, and bitwise the classes asked for one at a time."""
    model, gs = model_for(case), T.graphs_of(case)
    lref, oref = T.lesion_reference(case), T.occlusion_reference(case)
    sets = [r.sets for r in lref]
    single_l = {c: LES.run(model, gs, sets, classes=(c,)) for c in range(11)}
    single_o = {c: OCC.run(model, gs, classes=(c,)) for c in range(11)}
    worst = bound = 0.0
    for cl in T.CLASS_LISTS:
        got = LES.run(model, gs, sets, classes=cl)
        occ = OCC.run(model, gs, classes=cl)
        for d, (r, o) in enumerate(zip(lref, oref)):
            e, b = check_lesion(got, d, r.base64, r.base32, r.les64, r.les32, r.want_nan, classes=cl)
            e = max(e, check_occlusion(occ, d, r.base64, b, o, classes=cl))
            if e / b > worst / max(bound, 1e-30) or bound == 0.0:
                worst, bound = e, b
            for ci, c in enumerate(cl):
                assert got[1][ci, d] == single_l[c][1][0, d] and occ[1][ci, d] == single_o[c][1][0, d]
                assert np.array_equal(got[2][d][:, ci], single_l[c][2][d][:, 0], equal_nan=True), (cl, c, d)
                assert np.array_equal(occ[2][d][:, ci], single_o[c][2][d][:, 0], equal_nan=True), (cl, c, d)
    print("%s: worst %.2e under %.2e" % (case.id, worst, bound))
