"""Containers with another decoder than the published one (tests/decoder_variants.py), without a GPU: the builder, the two
conditions that let the suite's bounds carry over to a variant (they are conditions on the INPUTS of tests/test_decoder_containers_gpu.py,
not measurements of the code under test: a variant that breaks one is replaced, the bound stays), and every image the C++ packer makes
of a variant -- the recurrent image and the table rows through the lane-accurate recurrence step, W_ih inside the F(4,3) image through
the lane-accurate frontend program, each against float64 on the variant's own tensors.  (The two bf16 x 9 images: the container
parameter of tests/test_packing_emulation.py.)"""
import numpy as np
import pytest

import decoder_variants as dv
import emu_wave as E
from conftest import SRS, state_err

TAGS = ["16k", "8k"]


@pytest.fixture(scope="module")
def oracles(built, tmp_path_factory):
    from oracle import Oracle
    d = tmp_path_factory.mktemp("decoder_containers")
    return {name: Oracle(weights_path=dv.write_variant(name, d)) for name in ("published",) + dv.VARIANTS}


# ---- the builder --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dv.VARIANTS)
def test_variant_differs_from_the_published_container_only_in_its_decoder_tensors(name):
    from silero_vad_amd.tuning import DECODER_NAMES, _container_index, _prefix
    pub, blob = dv.published_blob(), dv.variant_blob(name)
    assert len(blob) == len(pub)
    a, b = np.frombuffer(pub, np.uint8), np.frombuffer(blob, np.uint8)
    may = np.zeros(len(pub), bool)
    index = _container_index(pub)
    for sr in dv.RATES:
        if dv.variant_tensors(name, sr) is None:
            continue
        for k in DECODER_NAMES:
            off, cnt, _ = index[_prefix(sr) + k]
            may[off:off + 4 * cnt] = True
            assert (a[off:off + 4 * cnt] != b[off:off + 4 * cnt]).any(), (sr, k)       # every tensor it means to change did change
    assert may.sum() == 4 * (2 * 128 * 512 + 2 * 512 + 128 + 1) * sum(dv.variant_tensors(name, sr) is not None for sr in dv.RATES)
    assert np.array_equal(a[~may], b[~may])
    assert _container_index(blob) == index


@pytest.mark.parametrize("name", dv.VARIANTS)
def test_variant_holds_what_was_put_in_and_builds_the_same_bytes_twice(name):
    from silero_vad_amd.tuning import DECODER_TENSORS, decoder_state_dict
    blob = dv.variant_blob(name)
    assert dv.build_variant(name) == blob and dv.build_variant(name) is not blob
    pub = dv.published_blob()
    for sr in dv.RATES:
        put = dv.variant_tensors(name, sr)
        want = decoder_state_dict(pub, sr) if put is None else put
        got = decoder_state_dict(blob, sr)
        assert list(got) == [k for k, _ in DECODER_TENSORS]
        for k, shape in DECODER_TENSORS:
            assert got[k].dtype == np.float32 and got[k].shape == shape
            assert np.array_equal(got[k].view(np.uint32).ravel(), np.asarray(want[k], np.float32).view(np.uint32).ravel()), (sr, k)
    if name == "swapped":
        for k, _ in DECODER_TENSORS:
            assert np.array_equal(decoder_state_dict(blob, 16000)[k], decoder_state_dict(pub, 8000)[k])
            assert np.array_equal(decoder_state_dict(blob, 8000)[k], decoder_state_dict(pub, 16000)[k])
    if name == "random":                                        # nothing of the published decoder is left in it
        for sr in dv.RATES:
            for k, _ in DECODER_TENSORS:
                assert not (decoder_state_dict(blob, sr)[k] == decoder_state_dict(pub, sr)[k]).any(), (sr, k)


# ---- the conditions on the variants ---------------------------------------------------------------------------------------------------------
COND_B, COND_T = 16, 32            # 16 rolled rows of the fixture, 32 chunks: four times the longest run the GPU file carries a state over


def _cond_rows(golden, tag):
    sr = SRS[tag]
    n = dv.chunk_of(sr)
    rows = dv.rolled_rows(golden[tag]["wav"], COND_B, COND_T * n, 3571)
    st0, cx0 = dv.carried(COND_B, COND_T, n)
    return sr, n, rows, st0, cx0


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ("published",) + dv.VARIANTS)
def test_condition_state_perturbation_does_not_grow(oracles, golden, name, tag):
    """The recurrence under the variant stays contracting: a change of the carried state by 1e-6 (max norm) moves the oracle's state by
    at most 64 x that after GPU_MAX_T chunks and after 32 (kept variants: at most 27 x; the rejected candidates -- `random` at the
    full sigma of weight_hh, the published decoder x 3 -- 263 x at T = 32 and 600 x at T = 8).  Otherwise two correct fp32 evaluations
    drift apart and a bound against the oracle means nothing."""
    sr, n, rows, st0, cx0 = _cond_rows(golden, tag)
    assert dv.GPU_MAX_T <= COND_T
    eps = 1e-6
    d = (eps * np.sign(np.random.default_rng(1).standard_normal(st0.shape))).astype(np.float32)
    for T in (dv.GPU_MAX_T, COND_T):
        _, _, a = oracles[name].forward_audio(rows[:, :T * n], sr, ctx=cx0, state=st0)
        _, _, b = oracles[name].forward_audio(rows[:, :T * n], sr, ctx=cx0, state=st0 + d)
        grow = float(np.abs(a.astype(np.float64) - b).max()) / eps
        print(f"{name} {tag} T={T}: state moves by {grow:.1f} x the perturbation")
        assert grow <= 64.0, (name, tag, T, grow)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ("published",) + dv.VARIANTS)
def test_condition_oracle_decoder_is_float64_accurate(oracles, golden, name, tag):
    """The reference of the GPU file is itself right on the variant: the oracle's decoder, fed its own encoder output (stage enc3),
    against the float64 numpy decoder on the variant's tensors carried over the same 32 chunks -- below 1e-6 on every probability and
    5e-6 (state_err) on the state after GPU_MAX_T and after 32 chunks."""
    sr, n, rows, st0, cx0 = _cond_rows(golden, tag)
    dec = dv.Decoder64(dv.decoder_of(name, sr))
    h, c = st0[0].astype(np.float64), st0[1].astype(np.float64)
    st, ctx = st0.copy(), cx0.copy()
    worst_p = 0.0
    for t in range(COND_T):
        x1 = np.concatenate([ctx, rows[:, t * n:(t + 1) * n]], 1)
        prob, st, stages = oracles[name].step(x1, st, sr, stages=True)
        ctx = x1[:, -(n // 8):]
        p64, h, c = dec.cell(dec.gates(stages["enc3"][:, :, 0]), h, c)
        worst_p = max(worst_p, float(np.abs(prob - p64).max()))
        if t + 1 in (dv.GPU_MAX_T, COND_T):
            se = state_err(st, np.stack([h, c]))
            print(f"{name} {tag} T={t + 1}: oracle decoder vs float64 |dp| {worst_p:.2e} state_err {se:.2e}")
            assert se < 5e-6, (name, tag, t + 1, se)
    assert worst_p < 1e-6, (name, tag, worst_p)


@pytest.mark.parametrize("tag", TAGS)
def test_random_variant_does_not_saturate(oracles, golden, tag):
    """`random`'s probabilities spread over the sigmoid's steep part where the published ones sit at 0 and 1: an error in h or in the
    head shows in the probability."""
    sr, n, rows, st0, cx0 = _cond_rows(golden, tag)
    p, _, _ = oracles["random"].forward_audio(rows, sr, ctx=cx0, state=st0)
    assert 0.01 < p.min() and p.max() < 0.99 and p.max() - p.min() > 0.5
    q, _, _ = oracles["published"].forward_audio(rows, sr, ctx=cx0, state=st0)
    assert q.max() > 0.999


# ---- the packed images of every variant -------------------------------------------------------------------------------------------------------
def dense_to_d(pre):
    """[16 streams][512 gate rows] -> the D-fragment order of the gate pre-activations, [32][4][64] (emu_wave.rec_step)"""
    gx = np.zeros((32, 4, 64), np.float32)
    lane = np.arange(64)
    for q in range(4):
        for w in range(8):
            for r in range(4):
                gx[8 * q + w, r] = pre[lane & 15, 128 * q + 16 * w + 4 * (lane >> 4) + r]
    return gx


def d_to_dense(gx):
    return np.concatenate([E.chain_to_dense(gx[8 * q:8 * q + 8]) for q in range(4)], 1)


def test_d_fragment_order_round_trip():
    pre = np.random.default_rng(0).standard_normal((16, 512)).astype(np.float32)
    assert np.array_equal(d_to_dense(dense_to_d(pre)), pre)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", dv.BOTH_RATES)
def test_recurrent_image_and_table_rows_of_a_variant(built, golden, name, tag):
    """rec_kernel's step (emu_wave.rec_step) on the variant's recurrent image (which 1) and table rows (which 2: w_out, b_out), from the
    golden carried state, with the gate pre-activations computed in float64 from the golden encoder output and the variant's weight_ih
    and biases: against the float64 LSTM step and head on the variant's tensors, at this suite's emulation bounds."""
    sr, g = SRS[tag], golden[tag]
    Q = 32 if sr == 16000 else 16
    im = dv.packed_images(name)
    dec = dv.Decoder64(dv.decoder_of(name, sr))
    pre = dec.gates(g["stage_enc3"][:, :, 0])
    h0, c0 = g["stage_state_in"][0], g["stage_state_in"][1]
    prob, hn, cn = E.rec_step(im[sr, 1], im[sr, 2], E.Tab(8 * Q, Q), dense_to_d(pre.astype(np.float32)), h0, c0)
    p64, h64, c64 = dec.cell(pre, h0.astype(np.float64), c0.astype(np.float64))
    assert np.abs(prob - p64).max() < 1e-5
    assert state_err(np.stack([hn, cn]), np.stack([h64, c64])) < 2e-5
    # ... and it is the variant's step, not the published decoder's
    pub = dv.Decoder64(dv.decoder_of("published", sr))
    _, hp, _ = pub.cell(pub.gates(g["stage_enc3"][:, :, 0]), h0.astype(np.float64), c0.astype(np.float64))
    assert np.abs(hp - h64).max() > 1e-2


@pytest.fixture(scope="module")
def published_f43(built, golden):
    out = {}
    for tag, sr in SRS.items():
        im = dv.packed_images("published")
        out[tag] = E.FrontF43Emu(sr, im[sr, 6], im[sr, 2]).run(golden[tag]["stage_x"])
    return out


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", dv.BOTH_RATES)
def test_f43_image_of_a_variant_carries_its_weight_ih(built, golden, published_f43, name, tag):
    """front_f43_kernel's program on the variant's F(4,3) image (which 6) and tables (which 2: the gate bias rows): the gate
    pre-activations against the program's own encoder output times the variant's weight_ih plus both biases in float64, at the
    direct-versus-Winograd bound of tests/test_packing_emulation.py; the encoder output is the published image's, bit for bit (the
    encoder units did not move)."""
    sr, g = SRS[tag], golden[tag]
    im = dv.packed_images(name)
    out = E.FrontF43Emu(sr, im[sr, 6], im[sr, 2]).run(g["stage_x"])
    assert np.array_equal(out["feat"].view(np.uint32), published_f43[tag]["feat"].view(np.uint32))
    want = dv.Decoder64(dv.decoder_of(name, sr)).gates(E.chain_to_dense(out["feat"]))
    got = d_to_dense(out["gx"])
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max())
    assert np.abs(got - d_to_dense(published_f43[tag]["gx"])).max() > 1e-2


@pytest.mark.parametrize("name", ["only16k", "only8k"])
def test_one_rate_variants_leave_the_other_rate_alone(built, name):
    """Every image of the rate the variant does not touch is the published image byte for byte, every image of the other rate is
    `random`'s -- and at that rate every image that holds a decoder tensor differs from the published one."""
    im, pub, rnd = dv.packed_images(name), dv.packed_images("published"), dv.packed_images("random")
    new = 16000 if name == "only16k" else 8000
    for sr in dv.RATES:
        for which in dv.WHICH:
            same_as = rnd if sr == new else pub
            assert np.array_equal(im[sr, which].view(np.uint32), same_as[sr, which].view(np.uint32)), (sr, which)
            if sr == new:
                assert not np.array_equal(im[sr, which].view(np.uint32), pub[sr, which].view(np.uint32)), (sr, which)
