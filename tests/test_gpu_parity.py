"""GPU (-m gpu): the HIP engine, called through the C ABI (mellow_amd.engine -> libmellow_hip.so), against
 (a) the golden vectors generated from the imported reference (tests/golden/*.npz), and
 (b) the CPU oracle on the same seeded inputs,
plus size-independent properties at the full BASELINE size (B=32, max_len=64).

Tolerances (fp32 path, exact-fp32 MFMA): activations rel 2e-4 of the tensor's max (fp32 summation-order noise of
deep K=96..4608 reductions); last-position logits atol 3e-3 on logits of std ~24; token ids EXACT (greedy)."""
import os

import numpy as np
import pytest
import torch

from mellow_amd import spec, synth

pytestmark = pytest.mark.gpu


def _close(got, ref, rel=2e-4, atol=0.0, name=""):
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    d = float((got - ref).abs().max())
    lim = atol + rel * float(ref.abs().max())
    assert d <= lim, f"{name}: max|d| {d:.3e} > {lim:.3e}"


# Every test that takes `engine` runs twice: on the exact fp32 MFMA path ("f32") and on the fp32-accurate bf16-split path
# ("f32x3": each fp32 operand is the exact sum of three bf16 terms, six bf16 MFMA products per fp32 product, fp32
# accumulation -- DESIGN.md 6c).  Both are held to the SAME tolerances and to exact token equality with the reference goldens.
@pytest.fixture(scope="module", params=["f32", "f32x3"])
def engine(request, synth_sd):
    from mellow_amd.engine import Engine
    e = Engine(device=0, precision=request.param)      # raises (does not fall back) without GPU / library
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine_f32(synth_sd):
    """the exact-fp32 engine, for tests that compare another mode against it or are precision-independent"""
    from mellow_amd.engine import Engine
    e = Engine(device=0, precision="f32")
    e.load_state_dict(synth_sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch2():
    return synth.make_batch(2)


@pytest.fixture(scope="module")
def oracle_taps(synth_sd, batch2):
    from oracle import mellow_oracle as O
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    a1, a2, ids = batch2
    taps = {}
    with torch.no_grad():
        prefix = O.generate_prefix_inference(synth_sd, torch.from_numpy(a1), torch.from_numpy(a2), torch.from_numpy(ids), taps)
    return prefix, taps


def test_native_library_is_loaded(engine_f32):
    """the product path IS the HIP library: it must be mapped into this process"""
    maps = open("/proc/self/maps").read()
    assert "libmellow_hip.so" in maps
    assert engine_f32.lib.mellow_device_count() >= 1


def test_frontend_logmel(engine, batch2, oracle_taps, golden_dir):
    a1, _, _ = batch2
    _, t = oracle_taps
    g = np.load(os.path.join(golden_dir, "enc10.npz"))
    lm = engine.logmel(a1, apply_bn=False)
    assert lm.shape == (2, 1001, 64)                       # frame / mel-bin layout: 320000/320 + 1 frames x 64 bins
    _close(lm, t["logmel"][:, 0], rel=2e-6, atol=5e-5, name="logmel vs oracle")
    _close(lm, g["logmel"], rel=2e-6, atol=5e-5, name="logmel vs reference golden")
    lmb = engine.logmel(a1, apply_bn=True)
    _close(lmb, t["logmel_bn"][:, 0], rel=5e-6, atol=1e-5, name="logmel_bn vs oracle")
    _close(lmb[:, ::10], g["logmel_bn_sub"], rel=5e-6, atol=1e-5, name="logmel_bn vs golden")


def test_encoder_taps(engine, batch2, oracle_taps, golden_dir, synth_sd):
    a1, _, _ = batch2
    _, t = oracle_taps
    g = np.load(os.path.join(golden_dir, "enc10.npz"))
    engine.enable_taps(True)
    try:
        enc = engine.encode(a1)
        pw = engine.tap("power").reshape(2, 1001, 544)
        if engine.precision == "f32":
            _close(pw[:, :, :513], t["power"][:, 0], rel=2e-6, name="power")
        else:
            # f32x3 runs the STFT on exact bf16 splits: against the oracle's fp32 conv1d it is a DIFFERENT fp32 summation order of
            # 1024-term dot products (measured 2.5e-6 of max, bound 4e-6); against an fp64 STFT of the same weights it must be at
            # least as close as the oracle's own fp32 arithmetic is
            _close(pw[:, :, :513], t["power"][:, 0], rel=4e-6, name="power")
            from oracle import mellow_oracle as O
            kr, ki = O.ENC + "spectrogram_extractor.stft.conv_real.weight", O.ENC + "spectrogram_extractor.stft.conv_imag.weight"
            with torch.no_grad():
                p64 = O.stft_power({kr: synth_sd[kr].double(), ki: synth_sd[ki].double()}, torch.from_numpy(a1).double())[:, 0]
            err_hip = float((pw[:, :, :513].cpu().double() - p64).abs().max())
            err_ref = float((t["power"][:, 0].double() - p64).abs().max())
            assert err_hip <= err_ref, (err_hip, err_ref)
        assert float(pw[:, :, 513:].abs().max()) == 0.0     # padded bins come from zero weight rows
        patch = engine.tap("patch").reshape(2, 4096, 96)
        _close(patch, t["patch"], name="patch")
        _close(patch[:, g["tok_idx"]], g["patch_sub"], name="patch golden")
        for s, shp in enumerate([(2, 1024, 192), (2, 256, 384), (2, 64, 768), (2, 64, 768)]):
            st = engine.tap(f"stage{s}").reshape(shp)
            _close(st, t[f"stage{s}"], name=f"stage{s}")
        _close(engine.tap("stage2").reshape(2, 64, 768), g["stage2"], name="stage2 golden")
        _close(engine.tap("stage3").reshape(2, 64, 768), g["stage3"], name="stage3 golden")
        fpx = engine.tap("fpx").reshape(2, 32, 544)[:, :, :527]
        _close(fpx, t["framewise"][:, 0::32], name="framewise (32 distinct rows)")
        _close(fpx, g["framewise32"], name="framewise golden")
        emb = engine.tap("emb33").reshape(2, 33, 768)
        _close(emb[:, 0], t["latent"], name="latent")
        _close(emb, g["embedding33"], name="embedding33 golden")
        p33 = engine.tap("proj33").reshape(2, 33, 576)
        _close(p33, g["projected33"], name="projected33 golden")
        _close(enc, t["audio1_ds"], name="downsampled audio (129 rows)")
    finally:
        engine.enable_taps(False)


def test_stft_runs_as_fft_only_on_windowed_dft_weights(synth_sd):
    """f32x3 mode runs A1 (htsat.py:864) as a 1024-point FFT per frame when -- and only when -- the checkpoint's conv_real /
    conv_imag weights are window[n] * cos / sin(2 pi k n / 1024) (checked element by element at load).  (a) the FFT's power
    spectrum against an fp64 STFT built from the SAME weights, on noise, digital silence, an impulse and a full-scale square
    wave: 1e-6 of the maximum (an fp32 FFT is more accurate than a 1024-term fp32 dot product); (b) the exact-fp32 engine keeps
    the GEMM; (c) a checkpoint with ONE perturbed basis element falls back to the GEMM on its own weights and follows them."""
    from mellow_amd.engine import Engine
    from oracle import mellow_oracle as O
    kr, ki = O.ENC + "spectrogram_extractor.stft.conv_real.weight", O.ENC + "spectrogram_extractor.stft.conv_imag.weight"
    n = 320000
    rng = np.random.default_rng(5)
    sq = np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    imp = np.zeros(n, dtype=np.float32)
    imp[777] = 1.0
    wav = np.stack([rng.standard_normal(n).astype(np.float32) * 0.3, np.zeros(n, dtype=np.float32), imp, sq])

    def power_of(engine):
        engine.enable_taps(True)
        try:
            engine.logmel(wav)
            return engine.tap("power").reshape(4, 1001, 544).cpu().double()
        finally:
            engine.enable_taps(False)

    def p64_of(sd):
        with torch.no_grad():
            return O.stft_power({kr: sd[kr].double(), ki: sd[ki].double()}, torch.from_numpy(wav).double())[:, 0]

    e3 = Engine(device=0, precision="f32x3")
    e3.load_state_dict(synth_sd)
    assert e3.stft_is_fft()
    pw, p64 = power_of(e3), p64_of(synth_sd)
    assert float(pw[:, :, 513:].abs().max()) == 0.0
    for i in range(4):
        scale = float(p64[i].max())
        assert float((pw[i, :, :513] - p64[i]).abs().max()) <= 1e-6 * scale + 1e-30, i
    assert float(pw[1].abs().max()) == 0.0                                    # silence stays exactly zero
    e0 = Engine(device=0, precision="f32")
    e0.load_state_dict(synth_sd)
    assert not e0.stft_is_fft()
    sd = dict(synth_sd)
    w = sd[kr].clone()
    w[200, 0, 300] += 0.25                                                    # no longer a windowed DFT basis
    sd[kr] = w
    e3b = Engine(device=0, precision="f32x3")
    e3b.load_state_dict(sd)
    assert not e3b.stft_is_fft()
    pb, pb64 = power_of(e3b), p64_of(sd)
    assert float((pb[0, :, :513] - pb64[0]).abs().max()) <= 4e-6 * float(pb64[0].max())
    assert float((pb64[0, :, 200] - p64[0, :, 200]).abs().max()) > 1e-3 * float(p64[0].max())     # the perturbation is visible
    for e in (e3, e0, e3b):
        e.close()


def test_prefix(engine, batch2, oracle_taps, golden_dir):
    a1, a2, ids = batch2
    oprefix, _ = oracle_taps
    g = np.load(os.path.join(golden_dir, "enc10.npz"))
    pre = engine.prefix(a1, a2, ids)
    assert pre.shape == (2, spec.PREFIX_LEN, spec.D_PROJ)
    _close(pre, oprefix, name="prefix vs oracle")
    _close(pre, g["prefix"], name="prefix vs reference golden")
    # layout: sep rows (embedding of id 0) at 129 and 259, text embeddings from 260 (decoder.py:54) are exact copies
    pre = pre.cpu()
    ref = torch.from_numpy(g["prefix"])
    assert torch.equal(pre[:, 129], ref[:, 129]) and torch.equal(pre[:, 259], ref[:, 259])
    assert torch.equal(pre[:, 260:], ref[:, 260:])


def test_lm_prefill_and_decode_logits(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    prefix = torch.from_numpy(e["prefix"])
    l0 = engine.lm_prefill(prefix, reserve=16)
    _close(l0, g["logits_step0"], rel=0, atol=3e-3, name="prefill logits")
    assert engine.argmax(l0).cpu().tolist() == g["tokens"][:, 0].tolist()
    toks = g["tokens"]
    for i in range(1, toks.shape[1]):
        li = engine.lm_decode_step(toks[:, i - 1])
        _close(li[:, torch.from_numpy(g["sub_vocab"])], g["logits_sub"][i], rel=0, atol=3e-3, name=f"decode step {i}")
        assert li.argmax(-1).cpu().tolist() == toks[:, i].tolist()


def test_generate_tokens_match_reference(engine, batch2, golden_dir):
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    steps = int(g["steps"])
    toks, lens, n, ftm = engine.generate(a1, a2, ids, max_len=steps, top_p=0.8, temperature=1.0, stop_id=0)
    assert n == steps and np.array_equal(toks, g["tokens"])
    assert ftm > 0
    # sampling parameters never change the arg-max
    toks2, *_ = engine.generate(a1, a2, ids, max_len=steps, top_p=0.1, temperature=0.3, stop_id=0)
    assert np.array_equal(toks2, toks)
    # eager launches == hipGraph replay
    engine.set_graph(False)
    toks3, *_ = engine.generate(a1, a2, ids, max_len=steps, stop_id=0)
    engine.set_graph(True)
    assert np.array_equal(toks3, toks)


def test_stop_token_semantics(engine, batch2, golden_dir):
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    stop = int(g["eos_stop_id"])
    # B=1: the loop ends right after the stop id; the text is cut before it (wrapper.py:247-254)
    toks, lens, n, _ = engine.generate(a1[:1], a2[:1], ids[:1], max_len=12, stop_id=stop)
    assert n == len(g["eos_b1_tokens"]) + 1 and int(lens[0]) == len(g["eos_b1_tokens"])
    assert toks[0, : lens[0]].tolist() == g["eos_b1_tokens"].tolist() and toks[0, lens[0]] == stop
    # B=2: row 1 never produces it, so all 12 steps run; row 0 is cut at its stop id
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=12, stop_id=stop)
    assert n == 12 and lens.tolist() == g["eos_b2_len"].tolist()
    assert toks[0, : lens[0]].tolist() == g["eos_b2_row0"].tolist()
    assert toks[1, : lens[1]].tolist() == g["eos_b2_row1"].tolist()


def test_long_audio_seven_crop_path(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "long30.npz"))
    wav = synth.make_clip(int(g["clip_idx"]), int(g["n_samples"]))[None]
    engine.enable_taps(True)
    try:
        enc = engine.encode(wav)
        _close(enc, g["audio_ds"], name="30 s clip: downsampled projected embedding")
        _close(engine.tap("fpx").reshape(1, 32, 544)[:, :, :527], g["framewise32"], name="30 s framewise")
        _close(engine.tap("emb33").reshape(1, 33, 768)[:, 0], g["latent"], name="30 s latent")
    finally:
        engine.enable_taps(False)


def test_edge_shapes(engine, batch2):
    a1, a2, ids = batch2
    # max_len = 1: only the prefill token
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=1, stop_id=0)
    assert toks.shape == (2, 1) and n == 1
    # batch rows are independent: a ragged batch (B=3) reproduces the B=2 rows
    a1b, a2b, idsb = synth.make_batch(3)
    t3, *_ = engine.generate(a1b, a2b, idsb, max_len=6, stop_id=0, ignore_stop=True)
    t2, *_ = engine.generate(a1b[:2], a2b[:2], idsb[:2], max_len=6, stop_id=0, ignore_stop=True)
    assert np.array_equal(t3[:2], t2)
    with pytest.raises(Exception):
        engine.generate(a1[:, :1000], a2[:, :1000], ids, max_len=2)     # shorter than one STFT window


def test_full_size_properties(engine):
    """BASELINE configs[1] size (B=32, 2x10 s, max_len=64): properties that need no oracle run."""
    B, L = 32, 64
    a1, a2, ids = synth.make_batch(B)
    a1[5], a2[5], ids[5] = a1[3], a2[3], ids[3]             # duplicate example -> identical rows
    t, lens, n, ftm = engine.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True)
    assert t.shape == (B, L) and n == L
    assert (t >= 0).all() and (t < 49152).all()
    assert np.array_equal(t[5], t[3])
    t_again, *_ = engine.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True)
    assert np.array_equal(t, t_again)                        # bit-reproducible (no atomics, fixed reduction order)
    t_short, *_ = engine.generate(a1, a2, ids, max_len=16, stop_id=0, ignore_stop=True)
    assert np.array_equal(t_short, t[:, :16])                # KV-cache consistency: a longer run extends a shorter one
    # the first two examples are the golden ones
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "gen.npz"))
    assert np.array_equal(t[:2, : g["tokens"].shape[1]], g["tokens"])
    # reference stop semantics at full size: stop id := token row 0 produced at step 3
    stop = int(t[0, 3])
    ts, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=stop)
    assert int(lens[0]) == 3 and np.array_equal(ts[:, :n], t[:, :n])


def test_multi_row_block_batch(engine):
    """B = 40 (two 32-row blocks, the second ragged): every row must equal the same example run in a small batch."""
    a1, a2, ids = synth.make_batch(40)
    t40, *_ = engine.generate(a1, a2, ids, max_len=5, stop_id=0, ignore_stop=True)
    t_lo, *_ = engine.generate(a1[:3], a2[:3], ids[:3], max_len=5, stop_id=0, ignore_stop=True)
    t_hi, *_ = engine.generate(a1[35:40], a2[35:40], ids[35:40], max_len=5, stop_id=0, ignore_stop=True)
    assert np.array_equal(t40[:3], t_lo) and np.array_equal(t40[35:40], t_hi)


def test_multi_row_block_decode_logits_match_the_one_block_path(engine, engine_f32):
    """The decode step of a batch of more than 32 rows runs other kernels than one of up to 32 rows (f32x3 mode, round 5:
    `dec_qkv2x3_kernel` / `dec_gateup3_kernel` serve every row block with weights split once, activations pre-split by their
    producers, and the lm_head streams its weights once for all blocks; the reference's loop is batch-agnostic,
    wrapper.py:216-249).  LOGITS, not only tokens: rows 0, 1 (block 0), 40 (block 1) and 94, 95 (block 2, ragged: B = 96 is three
    blocks, 72 is two + a quarter) of a teacher-forced B = 96 / B = 72 run against the same examples run alone through the
    one-block kernels, prefill + 4 decode steps: <= 1e-3 in the f32x3 mode (another summation order), 3e-3 against the exact
    fp32 engine, arg-max equal."""
    for B, pick in ((96, [0, 1, 40, 94, 95]), (72, [0, 33, 70, 71])):
        a1, a2, ids = synth.make_batch(B)
        pre_big = engine.prefix(a1, a2, ids)
        sub = np.asarray(pick)
        _close(pre_big[sub], engine.prefix(a1[sub], a2[sub], ids[sub]), rel=1e-5, name="prefix rows: only the split-K summation order depends on the batch")
        pre_small = pre_big[torch.from_numpy(sub).to(pre_big.device)].clone()          # the LM sees the same rows either way
        l_small = engine.lm_prefill(pre_small, reserve=8).clone()
        l_f32 = engine_f32.lm_prefill(pre_small, reserve=8).clone()
        small_steps, f32_steps, toks = [l_small], [l_f32], []
        for i in range(4):
            tok = small_steps[-1].argmax(-1)
            toks.append(tok)
            small_steps.append(engine.lm_decode_step(tok).clone())
            f32_steps.append(engine_f32.lm_decode_step(tok).clone())
        l_big = engine.lm_prefill(pre_big, reserve=8)
        for i in range(5):
            if i:
                full = l_big.argmax(-1)                      # the other rows follow their own greedy tokens
                full[torch.from_numpy(sub).to(full.device)] = toks[i - 1]
                l_big = engine.lm_decode_step(full)
            got = l_big[torch.from_numpy(sub).to(l_big.device)]
            _close(got, small_steps[i], rel=0, atol=1e-3, name=f"B = {B}, step {i}: rows of the multi-block step vs the same rows alone")
            _close(got, f32_steps[i], rel=0, atol=3e-3, name=f"B = {B}, step {i}: vs the exact fp32 engine")
            assert torch.equal(got.argmax(-1), small_steps[i].argmax(-1))


def test_exact_fp32_mode_across_batch_sizes(engine_f32):
    """What MELLOW_PRECISION_F32 promises about the batch size (`include/mellow_hip.h`, ABI minor 1), pinned: the LM of a 72-row
    batch (two row blocks + a quarter) against the same rows run alone through the one-block kernels.  Encoder-side and prefill
    arithmetic does not depend on the batch: the PREFILL logits are equal bit for bit.  The decode step picks wave counts per
    launch by the number of row blocks (4-way against 12-way LDS reductions in the fused down + q/k/v launch, 8- against 16-row
    o_proj workgroups) -- another fp32 summation order, measured 9e-5 on the logits: asserted <= 5e-4 with equal arg-max, for
    3 teacher-forced steps; the attention keeps its two key splits at every batch size in this mode (kernels.h `dec_key_splits`)."""
    B, pick = 72, [0, 33, 70, 71]
    a1, a2, ids = synth.make_batch(B)
    pre_big = engine_f32.prefix(a1, a2, ids)
    sub = torch.from_numpy(np.asarray(pick)).to(pre_big.device)
    pre_small = pre_big[sub].clone()
    small = [engine_f32.lm_prefill(pre_small, reserve=8).clone()]
    for i in range(3):
        small.append(engine_f32.lm_decode_step(small[-1].argmax(-1)).clone())
    l_big = engine_f32.lm_prefill(pre_big, reserve=8)
    assert torch.equal(l_big[sub], small[0]), f"prefill: max |d| {float((l_big[sub] - small[0]).abs().max()):.3e}"
    for i in range(1, 4):
        full = l_big.argmax(-1)
        full[sub] = small[i - 1].argmax(-1)
        l_big = engine_f32.lm_decode_step(full)
        _close(l_big[sub], small[i], rel=0, atol=5e-4, name=f"f32 mode, decode step {i}: rows of the 72-batch vs the same rows alone")
        assert torch.equal(l_big[sub].argmax(-1), small[i].argmax(-1))


@pytest.fixture(scope="module")
def batch1024():
    return synth.make_batch(1024)


def test_large_batches_keep_every_row_and_stay_deterministic(engine, batch1024):
    """B = 300 (ten row blocks, the last ragged) and the largest batch one call takes, B = 1024 (32 row blocks, ~70 GB of
    activations + KV pages: sized for the 288 GB part): every row equals the same example in a 32-row batch, two calls agree."""
    a1, a2, ids = batch1024
    t32, *_ = engine.generate(a1[:32], a2[:32], ids[:32], max_len=6, stop_id=0, ignore_stop=True)
    for B in (300, 1024):
        tb, lens, n, _ = engine.generate(a1[:B], a2[:B], ids[:B], max_len=6, stop_id=0, ignore_stop=True)
        assert tb.shape == (B, 6) and n == 6 and (tb >= 0).all() and (tb < 49152).all()
        assert np.array_equal(tb[:32], t32)
        lo = B - 20
        t_hi, *_ = engine.generate(a1[lo:B], a2[lo:B], ids[lo:B], max_len=6, stop_id=0, ignore_stop=True)
        assert np.array_equal(tb[lo:B], t_hi)
        tb2, *_ = engine.generate(a1[:B], a2[:B], ids[:B], max_len=6, stop_id=0, ignore_stop=True)
        assert np.array_equal(tb, tb2)
    # one row more than a pass takes: the call runs it as a second pass (test_batches_beyond_1024_rows_run_as_passes has the
    # stop-rule case), fixed-length tokens are the same examples' tokens
    t1025, _, n, _ = engine.generate(np.concatenate([a1, a1[:1]]), np.concatenate([a2, a2[:1]]), np.concatenate([ids, ids[:1]]),
                                     max_len=6, stop_id=0, ignore_stop=True)
    assert t1025.shape == (1025, 6) and n == 6 and np.array_equal(t1025[:1024], tb) and np.array_equal(t1025[1024], tb[0])


@pytest.mark.parametrize("B,n_new", [(2, 90), (1, 1600)])
def test_long_context_decode_matches_independent_prefill(engine, golden_dir, B, n_new):
    """Contexts beyond one attention chunk (> 448 keys) up to 389 + 1600 = 1989 keys (five key
    chunks per split), checked against an independent implementation inside the engine: the prefill path (big GEMM + flash
    attention) run on the EXTENDED sequence must give the same last-position logits as the step-by-step KV-cached decode.
    (Up to 688 keys the decode is pinned against the reference itself: test_late_positions_match_reference.)"""
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    prefix = torch.from_numpy(e["prefix"])[:B]                   # (B, 389, 576)
    logits = engine.lm_prefill(prefix, reserve=n_new + 2)
    toks = []
    for i in range(n_new):
        t = logits.argmax(-1).to(torch.int32)
        toks.append(t.cpu())
        logits = engine.lm_decode_step(t)
    dec_logits = logits.cpu()
    toks = torch.stack(toks, 1).long()                           # (B, n_new)
    from mellow_amd import spec as _s
    sd_embed = synth.make_state_dict(0)[_s.LM + "model.embed_tokens.weight"]
    ext = torch.cat((prefix, sd_embed[toks]), 1)                 # (B, 389 + n_new, 576)
    pre_logits = engine.lm_prefill(ext, reserve=2).cpu()
    _close(dec_logits, pre_logits, rel=0, atol=3e-3, name=f"decode@{389 + n_new} vs prefill of the extended sequence")
    assert dec_logits.argmax(-1).tolist() == pre_logits.argmax(-1).tolist()


def test_max_len_at_the_page_limit(synth_sd, batch2, golden_dir):
    """max_len = everything the KV pages of an engine built with max_positions = 2048 can hold (2048 - 389 = 1659 steps): runs
    to the end, starts with the golden tokens, and a longer request is refused by the C ABI (the wrapper clamps with a warning
    instead: tests/test_tokenizer_cpu.py).  The default engine goes to the LM's own 8192 positions (next test)."""
    from mellow_amd.engine import Engine, EngineError
    a1, a2, ids = batch2
    e2k = Engine(device=0, precision="f32", max_positions=2048)
    e2k.load_state_dict(synth_sd)
    try:
        L = e2k.max_new_tokens_limit()
        assert L == 2048 - spec.PREFIX_LEN
        toks, lens, n, _ = e2k.generate(a1[:1], a2[:1], ids[:1], max_len=L, stop_id=-1)
        g = np.load(os.path.join(golden_dir, "late.npz"))
        assert n == L and toks.shape == (1, L) and np.array_equal(toks[0, :300], g["tokens"][0])
        assert (toks >= 0).all() and (toks < 49152).all()
        with pytest.raises(EngineError, match="exceeds max_positions 2048"):
            e2k.generate(a1[:1], a2[:1], ids[:1], max_len=L + 1, stop_id=-1)
    finally:
        e2k.close()


def test_max_len_3000_beyond_the_old_2048_key_cap(engine, golden_dir):
    """the reference's loop is bounded only by the LM's 8192 positions (wrapper.py:216, decoder.py:25); the
    engine's pages now grow with the request instead of clamping at 2048 keys.  One row, max_len = 3000 (contexts to 3389 keys,
    seven 448-key chunks per split): (a) the first 300 tokens are the reference's own (late.npz); (b) the KV-cached decode at
    the END of the run agrees with an independent implementation inside the engine -- the prefill path (big GEMMs + flash
    attention) run on the whole extended sequence gives the same last-position logits and the same next token."""
    assert engine.max_new_tokens_limit() == 8192 - spec.PREFIX_LEN
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    a1, a2, ids = synth.make_batch(1)
    L = 3000
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=-1)
    g = np.load(os.path.join(golden_dir, "late.npz"))
    assert n == L and toks.shape == (1, L) and np.array_equal(toks[0, :300], g["tokens"][0])
    prefix = torch.from_numpy(e["prefix"])[:1]
    sd_embed = synth.make_state_dict(0)[spec.LM + "model.embed_tokens.weight"]
    ext = torch.cat((prefix, sd_embed[torch.from_numpy(toks[:, : L - 1]).long()]), 1)       # (1, 389 + 2999, 576)
    pre_logits = engine.lm_prefill(ext, reserve=2).cpu()
    assert int(pre_logits.argmax(-1)) == int(toks[0, L - 1])
    # and step by step over the last stretch: teacher-forced decode from a 3300-key prefill reaches the same logits
    cut = 3300 - 389
    logits = engine.lm_prefill(ext[:, : 389 + cut], reserve=L - cut + 2)
    for i in range(cut, L - 1):
        assert int(logits.argmax(-1)) == int(toks[0, i]), i
        logits = engine.lm_decode_step(toks[:, i])
    _close(logits.cpu(), pre_logits, rel=0, atol=3e-3, name="decode@3388 keys vs prefill of the extended sequence")


def test_batches_beyond_1024_rows_run_as_passes(engine_f32, golden_dir):
    """one pass of the engine takes 1024 rows; `mellow_generate` runs a larger batch as consecutive passes.
    1030 rows under the reference stop rule: pass 0 (1024 rows cycling over examples that stop at steps 8 / 17 / 3 / never)
    runs to max_len, pass 1 (six copies of the example that stops at step 3) ends early; every row's tokens and length are the
    reference's (eos_mixed.npz), the columns pass 1 never computed are -1, the call reports the longest pass."""
    g = np.load(os.path.join(golden_dir, "eos_mixed.npz"))
    stop, L = int(g["stop_id"]), int(g["max_len"])
    ex = g["one_never_examples"].tolist()                    # (1, 2, 4, 3): stop at 8, 17, 3, never
    rows = [ex[i % 4] for i in range(1024)] + [ex[2]] * 6
    a1, a2, ids = synth.make_examples(ex)
    pick = [ex.index(r) for r in rows]
    toks, lens, n, _ = engine_f32.generate(a1[pick], a2[pick], ids[pick], max_len=L, stop_id=stop)
    assert toks.shape == (1030, L) and n == L
    want = {ex[i]: g[f"one_never_row{i}"] for i in range(4)}
    for r, e_ in enumerate(rows):
        assert int(lens[r]) == len(want[e_]) and toks[r, : lens[r]].tolist() == want[e_].tolist(), r
    assert (toks[1024:, 5:] == -1).all()                     # pass 1 stopped after step 3 (step 4 may still have been enqueued)
    free = g["one_never_free_tokens"][3]
    assert np.array_equal(toks[3, :L], free[:L])             # a row that never stops: the free-running reference tokens


def test_late_positions_match_reference(engine, batch2, golden_dir):
    """Contexts 389..688 (beyond one 448-key attention chunk, BASELINE config 3's max_len) against the REFERENCE's own
    300-step loop (tests/golden/late.npz: unmodified `_generate_batch`, no KV cache), not against the engine's prefill:
    (a) all 300 greedy token ids of both rows are equal (minimum reference top-2 gap over the run: 0.018);
    (b) teacher-forced with the reference's tokens, the last-position logits of steps 63 / 150 / 299 (T = 452 / 539 / 688)
        agree within the 3e-3 the fp32 path is held to everywhere else."""
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "late.npz"))
    ref = g["tokens"]
    L = int(g["steps"])
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True)
    assert n == L
    bad = np.argwhere(toks != ref)
    assert bad.size == 0, f"first divergence from the reference at (row, step) {bad[0].tolist()}"
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    logits = engine.lm_prefill(torch.from_numpy(e["prefix"]), reserve=L)
    keep = {int(k): j for j, k in enumerate(g["keep_steps"])}
    sub = torch.from_numpy(g["sub_vocab"])
    for i in range(1, L):
        logits = engine.lm_decode_step(ref[:, i - 1])
        if i in keep:
            _close(logits[:, sub], g["logits_sub"][keep[i]], rel=0, atol=3e-3, name=f"logits at step {i}")
            _close(logits.max(-1).values, g["logits_max"][keep[i]], rel=0, atol=3e-3, name=f"max logit at step {i}")
            assert logits.argmax(-1).cpu().tolist() == ref[:, i].tolist()


def test_all_position_forward_matches_reference(engine, batch2, golden_dir):
    """`Mellow.forward` (mellow.py:89-98 -> decoder.py:57-90, the training-time forward, inference arithmetic only): logits of
    EVERY position of [prefix | embed(answer)] against the reference's own `model(input_dict).logits` (tests/golden/forward.npz),
    through `mellow_embed_tokens` + `mellow_lm_forward_logits`; and consistency with the generation path (the last-position
    logits of prefill are the row T-1 of the same forward)."""
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "forward.npz"))
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    ans, f0 = g["answer_ids"], int(g["from_pos"])
    emb = engine.embed_tokens(ans)
    assert emb.shape == (2, ans.shape[1], 576)
    assert np.array_equal(emb[:, :, ::9].cpu().numpy(), g["answer_embed_sub"])          # a gather: bit-exact
    sub = torch.from_numpy(g["sub_vocab"])
    # (a) from the reference's prefix: isolates the LM
    seq = torch.cat((torch.from_numpy(e["prefix"]).to(emb.device), emb), 1)
    tail = engine.lm_forward_logits(seq, from_pos=f0)
    assert tail.shape == (2, seq.shape[1] - f0, 49152)
    _close(tail[:, :, sub], g["logits_sub"], rel=0, atol=3e-3, name="all-position logits (sub-vocabulary)")
    _close(tail.max(-1).values, g["logits_max"], rel=0, atol=3e-3, name="all-position max logit")
    assert np.array_equal(tail.argmax(-1).cpu().numpy(), g["argmax"])
    # (b) end to end from the waveforms, like the reference's forward(input_dict)
    tail2 = engine.forward(a1, a2, ids, ans, from_pos=f0)
    _close(tail2[:, :, sub], g["logits_sub"], rel=0, atol=3e-3, name="forward(input_dict) logits")
    # (c) from_pos = 0 returns every row; row T-1 of a prefix-only forward is what prefill hands to the decode loop
    pre = torch.from_numpy(e["prefix"])
    full = engine.lm_forward_logits(pre[:1], from_pos=0)
    assert full.shape == (1, 389, 49152)
    last = engine.lm_prefill(pre[:1])
    _close(full[:, -1], last, rel=0, atol=2e-3, name="row T-1 vs prefill logits")
    # (d) the all-position forward leaves no decode state behind, and does not disturb a later generate
    from mellow_amd.engine import EngineError
    engine.lm_forward_logits(pre[:1], from_pos=388)
    with pytest.raises(EngineError):
        engine.lm_decode_step(np.zeros(1, dtype=np.int64))
    gg = np.load(os.path.join(golden_dir, "gen.npz"))
    toks, _, _, _ = engine.generate(a1, a2, ids, max_len=8, stop_id=-1)
    assert np.array_equal(toks, gg["tokens"][:, :8])
    with pytest.raises(EngineError):                     # a generate call's decode state is not a base for the step tap either
        engine.lm_decode_step(np.zeros(2, dtype=np.int64))
    with pytest.raises(EngineError):
        engine.lm_forward_logits(pre[:1], from_pos=389)
    with pytest.raises(IndexError):
        engine.embed_tokens(np.array([49152]))
    # (e) the reference model object's call surface: model(input_dict).logits, model.generate_prefix_inference(input_dict)
    d = {"audio1": torch.from_numpy(a1), "audio2": torch.from_numpy(a2), "input": {"input_ids": torch.from_numpy(ids)},
         "answer": {"input_ids": torch.from_numpy(ans)}}
    out = engine(d)
    assert out.loss is None and out.logits.shape == (2, 389 + ans.shape[1], 49152)
    _close(out.logits[:, f0:, sub], g["logits_sub"], rel=0, atol=3e-3, name="model(input_dict).logits")
    pfx, _, _ = engine.generate_prefix_inference(d)
    _close(pfx, e["prefix"], name="generate_prefix_inference(input_dict)")


def test_batch32_matches_reference(engine, golden_dir):
    """BASELINE configs[1]'s batch -- the 32 examples `bench.py` times -- against the REFERENCE run on the same 32 examples
    (tests/golden/b32.npz: unmodified `generate_prefix_inference` + `_generate_batch` for ALL 64 steps of max_len = 64 -- the
    whole benchmarked run; minimum top-2 gap 0.0115): the 32 x 64 token matrix is equal, every row's prefix agrees, and
    teacher-forced with the reference's tokens (so a late divergence cannot hide an early one) the maximum logit of every row
    at every step and the sub-vocabulary logits of steps 0..7, 15, 23, ..., 63 agree within the 3e-3 of the fp32 path."""
    g = np.load(os.path.join(golden_dir, "b32.npz"))
    a1, a2, ids = synth.make_batch(32)
    steps = int(g["steps"])
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=steps, stop_id=-1)
    bad = np.argwhere(toks != g["tokens"])
    assert n == steps and bad.size == 0, f"first divergence from the reference at (row, step) {bad[0].tolist()}"
    pre = engine.prefix(a1, a2, ids)
    _close(pre[:, ::7, ::5], g["prefix_sub"], name="prefix of all 32 rows (sub-sampled)")
    sub = torch.from_numpy(g["sub_vocab"])
    assert steps == 64 and g["tokens"].shape == (32, 64)
    kept = {int(s): k for k, s in enumerate(g["logit_steps"])}
    logits = engine.lm_prefill(pre, reserve=steps)
    for i in range(steps):
        if i:
            logits = engine.lm_decode_step(g["tokens"][:, i - 1])
        if i in kept:
            _close(logits[:, sub], g["logits_sub"][kept[i]], rel=0, atol=3e-3, name=f"logits of 32 rows at step {i}")
        _close(logits.max(-1).values, g["logits_max"][i], rel=0, atol=3e-3, name=f"max logit at step {i}")
        assert logits.argmax(-1).cpu().tolist() == g["tokens"][:, i].tolist()


@pytest.mark.parametrize("n_rows,n_early,min_repacks", [(64, 5, 1), (96, 6, 2), (40, 4, 1)])
def test_rows_migrate_between_blocks_when_most_have_stopped(engine_f32, golden_dir, n_rows, n_early, min_repacks):
    """SURVEY 8f-3, row compaction: 64 / 96 / 40 rows in 32-row blocks, n_early of every 8 of them copies of examples that produce the stop id at
    steps 2..6 (tests/golden/b32.npz: the reference's own tokens for examples 4, 9, 14, 22, 24, 26), spread over BOTH blocks.
    Once they have stopped, the 24 running rows fit into one block: they are repacked into block 0 and block 1's kernels
    return at once.  Every row's tokens up to its own stop are those of the free-running reference tokens, rows that never
    stop run to the end, and the repack really happened (`mellow_last_row_repacks`)."""
    g = np.load(os.path.join(golden_dir, "b32.npz"))
    stop = 42274
    early = [4, 9, 14, 22, 24, 26]                   # first stop id at steps 3, 3, 3, 2, 6, 5
    late = [0, 1, 3, 7, 8, 12]                       # no stop id within the first 8 steps
    rows = []
    for i in range(n_rows):                          # n_early early rows, then late ones, through all the blocks
        rows.append(early[(i // 8 * 5 + i % 8) % 6] if i % 8 < n_early else late[(i // 8 * 3 + i % 8) % 6])
    a1, a2, ids = synth.make_examples(rows)
    L = 8
    toks, lens, n, _ = engine_f32.generate(a1, a2, ids, max_len=L, stop_id=stop)
    assert engine_f32.last_row_repacks() >= min_repacks
    ref = g["tokens"][:, :L]
    assert all(stop not in ref[e_] for e_ in late)
    for i, ex in enumerate(rows):
        want = ref[ex]
        hit = np.flatnonzero(want == stop)
        k = int(hit[0]) if hit.size else L
        assert int(lens[i]) == min(k, n), (i, ex, lens[i], k)
        m = min(k + 1, n)
        assert np.array_equal(toks[i, :m], want[:m]), (i, ex, toks[i], want)
        assert ((toks[i, m:n] == -1) | (toks[i, m:n] == want[m:n])).all()       # later columns: never computed, or the free run
    assert n == L                                    # the late rows never stop: the loop runs to max_len


def test_batch64_matches_reference(engine, golden_dir):
    """The north_star's batch of 64 in ONE call (two 32-row blocks): rows 0..31 against the reference's 32-example run
    (b32.npz), rows 32..63 against its run of examples 32..63 (b64tail.npz, 16 steps) -- tokens equal, prefixes and the per-step
    maximum logit (teacher-forced) within the fp32 path's tolerances."""
    g1 = np.load(os.path.join(golden_dir, "b32.npz"))
    g2 = np.load(os.path.join(golden_dir, "b64tail.npz"))
    a1, a2, ids = synth.make_batch(64)
    steps = int(g2["steps"])
    ref = np.concatenate([g1["tokens"][:, :steps], g2["tokens"]])
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=steps, stop_id=-1)
    bad = np.argwhere(toks != ref)
    assert n == steps and bad.size == 0, f"first divergence from the reference at (row, step) {bad[0].tolist()}"
    pre = engine.prefix(a1, a2, ids)
    _close(pre[:32, ::7, ::5], g1["prefix_sub"], name="prefix rows 0..31")
    _close(pre[32:, ::13, ::9], g2["prefix_sub"], name="prefix rows 32..63")
    logits = engine.lm_prefill(pre, reserve=steps)
    for i in range(steps):
        if i:
            logits = engine.lm_decode_step(ref[:, i - 1])
        want = np.concatenate([g1["logits_max"][i], g2["logits_max"][i]])
        _close(logits.max(-1).values, want, rel=0, atol=3e-3, name=f"max logit of 64 rows at step {i}")
        assert logits.argmax(-1).cpu().tolist() == ref[:, i].tolist()


def test_ragged_batch3_matches_reference(engine, golden_dir):
    """B = 3 run by the reference itself (tests/golden/ragged3.npz): tokens exact, third row's prefix and logits in tolerance."""
    g = np.load(os.path.join(golden_dir, "ragged3.npz"))
    a1, a2, ids = synth.make_examples(g["examples"].tolist())
    steps = int(g["steps"])
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=steps, stop_id=-1)
    assert n == steps and np.array_equal(toks, g["tokens"])
    pre = engine.prefix(a1, a2, ids)
    _close(pre[2], g["prefix_row2"], name="prefix of row 2")
    logits = engine.lm_prefill(pre, reserve=steps)
    sub = torch.from_numpy(g["sub_vocab"])
    for i in range(steps):
        _close(logits[:, sub], g["logits_sub"][i], rel=0, atol=3e-3, name=f"B=3 logits step {i}")
        if i + 1 < steps:
            logits = engine.lm_decode_step(g["tokens"][:, i])


class _IdTokenizer:
    """token-level stand-in used by the goldens: one word per id, the stop id rendered as the stop string"""

    def __init__(self, stop_id):
        self.stop_id = stop_id

    def encode(self, s):
        return [self.stop_id]

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(i) == self.stop_id else f"t{int(i)}" for i in np.atleast_1d(ids))


def test_mixed_eos_matches_reference_cut_rule(engine, synth_sd, golden_dir):
    """Rows that reach the stop id at different steps (reference wrapper.py:241-254, tests/golden/eos_mixed.npz):
    the loop ends right after the step at which the LAST row produced it, every row's text is cut at its own first stop id,
    and the engine enqueues at most one step past the deciding one (device-published progress word, no host sync)."""
    g = np.load(os.path.join(golden_dir, "eos_mixed.npz"))
    stop, L = int(g["stop_id"]), int(g["max_len"])
    for case in ("all_stop", "one_never"):
        rows = g[f"{case}_examples"].tolist()
        a1, a2, ids = synth.make_examples(rows)
        toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=stop)
        assert n == int(g[f"{case}_steps"]), (case, n)
        assert lens.tolist() == g[f"{case}_len"].tolist(), (case, lens)
        for r in range(len(rows)):
            assert toks[r, : lens[r]].tolist() == g[f"{case}_row{r}"].tolist(), (case, r)
        assert np.array_equal(toks[:, :n], g[f"{case}_free_tokens"][:, :n])      # stopping never changes a token
        assert n <= engine.last_steps_enqueued() <= min(L, n + 1), (case, n, engine.last_steps_enqueued())
    # the same through the wrapper's text path: one string per example, cut before the stop string
    from mellow_amd import MellowWrapper
    m = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=synth_sd, tokenizer=_IdTokenizer(stop))
    rows = g["all_stop_examples"].tolist()
    a1, a2, ids = synth.make_examples(rows)
    got = m._generate_batch(torch.from_numpy(a1), torch.from_numpy(a2), torch.from_numpy(ids), entry_length=L)
    want = [" ".join(f"t{int(t)}" for t in g[f"all_stop_row{r}"]) for r in range(len(rows))]
    assert [s.strip() for s in got] == want
    m.model.close()


def test_wrapper_without_keywords_runs_the_benchmarked_mode(synth_sd, golden_dir, monkeypatch):
    """`MellowWrapper("v0", "v0", 0)` with no precision keyword runs the mode bench.py's `dtype` names
    (f32x3, the library's default), and that mode gives the reference's tokens."""
    from mellow_amd import MellowWrapper
    from mellow_amd.engine import DEFAULT_PRECISION, Engine
    monkeypatch.delenv("MELLOW_PRECISION", raising=False)
    m = MellowWrapper("v0", "v0", 0, state_dict=synth_sd, tokenizer=_IdTokenizer(-1))      # state_dict / tokenizer: offline stand-ins
    assert m.model.precision == DEFAULT_PRECISION == "f32x3"
    assert Engine.__init__.__defaults__[-1] is None
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    a1, a2, ids = synth.make_batch(2)
    toks, *_ = m.model.generate(a1, a2, ids, max_len=int(g["steps"]), stop_id=-1)
    assert np.array_equal(toks, g["tokens"])
    m.model.close()


def test_row_block_early_exit(engine, golden_dir):
    """B = 40 = two 32-row blocks under the reference stop rule: block 0 holds 32 copies of an example that produces the stop
    id at step 3, block 1 rows that stop at steps 8 / 17 / never.  After step 3 block 0 is no longer computed (its columns stay
    -1), block 1 is unaffected (tokens == the reference's), lengths follow the reference cut rule."""
    g = np.load(os.path.join(golden_dir, "eos_mixed.npz"))
    stop, L = int(g["stop_id"]), int(g["max_len"])
    ex = g["one_never_examples"].tolist()                    # (1, 2, 4, 3): stop at 8, 17, 3, never
    rows = [ex[2]] * 32 + [ex[0], ex[1], ex[3], ex[0], ex[1], ex[3], ex[0], ex[1]]
    a1, a2, ids = synth.make_examples(rows)
    toks, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=stop)
    assert n == L                                            # the "never" rows keep the loop alive to max_len
    want = {ex[i]: g[f"one_never_row{i}"] for i in range(4)}
    free = {ex[i]: g["one_never_free_tokens"][i] for i in range(4)}
    for r, e_ in enumerate(rows):
        assert int(lens[r]) == len(want[e_]) and toks[r, : lens[r]].tolist() == want[e_].tolist(), r
    assert np.array_equal(toks[:32, :4], np.tile(free[ex[2]][:4], (32, 1)))
    assert (toks[:32, 5:] == -1).all()                       # block 0 stopped being computed (step 4 may still run)
    for r in range(32, 40):
        assert np.array_equal(toks[r], free[rows[r]][:L]), r
    # the fixed-length mode never skips
    t2, *_ = engine.generate(a1, a2, ids, max_len=8, stop_id=stop, ignore_stop=True)
    assert (t2 >= 0).all() and np.array_equal(t2[:32], np.tile(free[ex[2]][:8], (32, 1)))


def test_stop_at_first_token_and_nan_audio(engine, batch2, golden_dir):
    """Edges of the loop: (a) every row produces the stop id at step 0 -> one iteration, empty texts;
    (b) a NaN sample poisons its row only: torch.argmax treats NaN as the maximum, so that row decodes id 0 for ever
        (first NaN), nothing faults, and the other row is untouched."""
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    t0 = int(g["tokens"][0, 0])
    toks, lens, n, _ = engine.generate(a1[:1], a2[:1], ids[:1], max_len=9, stop_id=t0)
    assert n == 1 and lens.tolist() == [0] and engine.last_steps_enqueued() <= 2
    bad = a1.copy()
    bad[0, 1000] = np.nan
    toks, lens, n, _ = engine.generate(bad, a2, ids, max_len=4, stop_id=-1)
    assert toks[0].tolist() == [0, 0, 0, 0]
    assert toks[1].tolist() == g["tokens"][1, :4].tolist()
    # ... and the poisoned request leaves nothing behind: the NaN K/V it appended beyond the next call's context are
    # masked by value, not only by weight
    toks, *_ = engine.generate(a1, a2, ids, max_len=4, stop_id=-1)
    assert np.array_equal(toks, g["tokens"][:, :4])
    with pytest.raises(IndexError):
        engine.generate(a1, a2, np.full_like(ids, 49152), max_len=2)
    # ids that are already device int32 (the timed path: no torch kernel, no host sync) are range-checked ON the device: the
    # prefix kernel flags the call's error word, the C call fails with the reference's IndexError text, nothing is left behind
    for bad_id in (49152, -3, 2 ** 31 - 1):
        dev_ids = torch.from_numpy(ids).to(engine.tdev, torch.int32)
        dev_ids[1, 5] = bad_id
        with pytest.raises(IndexError, match="index out of range in self"):
            engine.generate(a1, a2, dev_ids, max_len=2)
        with pytest.raises(IndexError):
            engine.prefix(a1, a2, dev_ids)
    big = torch.from_numpy(ids).to(engine.tdev)                     # int64 on the device: 2^32 + 5 must not alias id 5
    big[0, 0] = 2 ** 32 + 5
    with pytest.raises(IndexError):
        engine.generate(a1, a2, big, max_len=2)
    toks, *_ = engine.generate(a1, a2, torch.from_numpy(ids).to(engine.tdev, torch.int32), max_len=4, stop_id=-1)
    assert np.array_equal(toks, g["tokens"][:, :4])


def test_max_len_values_share_one_graph_and_any_out_buffer(engine, batch2, golden_dir):
    """The decode graphs depend on neither the caller's output tensor, nor max_len inside a 64-position bucket, nor the
    stop id: results stay equal to the goldens across such calls."""
    a1, a2, ids = batch2
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    for L, stop in ((12, 0), (10, 5), (12, 7), (11, 0)):
        toks, *_ = engine.generate(a1, a2, ids, max_len=L, stop_id=stop, ignore_stop=True)
        assert np.array_equal(toks, g["tokens"][:, :L])


class _StubTokenizer:
    """Deterministic stand-in for the SmolLM2 tokenizer (its files cannot be fetched offline): one id per
    whitespace-separated word (stable hash into 17..49151), '!' is the pad id 1, '<|endoftext|>' is id 0."""
    pad_id, eos_id = 1, 0

    def _word(self, w):
        if w == "<|endoftext|>":
            return self.eos_id
        h = 2166136261
        for c in w.encode():
            h = ((h ^ c) * 16777619) & 0xFFFFFFFF
        return 17 + h % (49152 - 17)

    def encode(self, text):
        return [self._word(w) for w in text.split()]

    def encode_plus(self, text, add_special_tokens=True, truncation=True, max_length=129, padding="max_length",
                    return_tensors="pt"):
        ids = self.encode(text)[:max_length]
        mask = [1] * len(ids) + [0] * (max_length - len(ids))
        ids = ids + [self.pad_id] * (max_length - len(ids))
        return {"input_ids": torch.tensor([ids]), "attention_mask": torch.tensor([mask])}

    def decode(self, ids):
        return " ".join("<|endoftext|>" if int(i) == self.eos_id else f"t{int(i)}" for i in ids)


def _write_wav16(path, x, sr):
    import wave
    pcm = (np.clip(x, -1, 1) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def test_wrapper_end_to_end_from_wav_files(synth_sd, tmp_path):
    """BASELINE config 1 shape (example.py flow): two wav files + a prompt through MellowWrapper.generate on the GPU
    == the oracle driven with the SAME preprocessed arrays and ids (44.1 kHz file -> resample -> tile; 32 kHz file)."""
    from mellow_amd import MellowWrapper
    from mellow_amd.audio import load_audio_into_tensor
    from oracle import mellow_oracle as O
    rng = np.random.default_rng(5)
    t1 = np.arange(int(3.3 * 44100)) / 44100.0
    x1 = 0.3 * np.sin(2 * np.pi * 440 * t1) + 0.05 * rng.standard_normal(t1.size)
    t2 = np.arange(int(10.0 * 32000)) / 32000.0
    x2 = 0.2 * np.sin(2 * np.pi * 1250 * t2) * np.sin(2 * np.pi * 3 * t2) + 0.05 * rng.standard_normal(t2.size)
    p1, p2 = tmp_path / "a.wav", tmp_path / "b.wav"
    _write_wav16(p1, x1, 44100)
    _write_wav16(p2, x2, 32000)
    tok = _StubTokenizer()
    m = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=synth_sd, tokenizer=tok)
    prompt = "what is the difference between the two audios"
    examples = [[str(p1), str(p2), prompt], [str(p2), str(p1), "describe both"]]
    got = m.generate(examples=examples, max_len=10, top_p=0.8, temperature=1.0)
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(s, str) for s in got)

    a1 = torch.cat([load_audio_into_tensor(str(p), 10, 32000, True).reshape(1, -1) for p in (p1, p2)], 0)
    a2 = torch.cat([load_audio_into_tensor(str(p), 10, 32000, True).reshape(1, -1) for p in (p2, p1)], 0)
    ids = torch.cat([tok.encode_plus(p, max_length=spec.TEXT_LEN)["input_ids"] for p in (prompt, "describe both")], 0)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        prefix = O.generate_prefix_inference(synth_sd, a1, a2, ids)
        toks = O.generate_batch(synth_sd, O.LMParams(), prefix, 10, 0.8, 1.0, tok.eos_id)
    want = [tok.decode(r).split("<|endoftext|>")[0] for r in np.asarray(toks)]
    assert got == want
    m.model.close()


# (row, first differing step) of the 32 x 300 run against the reference's own run (b32long.npz), per precision mode, as measured
# on MI355X this round; every entry is one of the reference's nine near-ties (gap < 6e-3).  Token-exact decisions: 9600 minus
# the tails of these rows.
_B32LONG_DEPARTURES = {"f32": {(10, 153)}, "f32x3": {(10, 153)}}


def test_config3_shape_max_len_300_sampling_args(engine, golden_dir):
    """BASELINE configs[2] at its exact per-rank shape: 32 examples, top_p=0.8, temperature=1.0, max_len=300 (context 389..689).
    The 32 x 300 tokens are held to the REFERENCE's own 300-step run of the 32 examples (b32long.npz: the imported reference's
    unmodified loop, 1 h 45 min on the build container; equality up to the reference's own near-ties, see below), and teacher-forced with its tokens the maximum logit of every row agrees
    within 3e-3 at steps 63 / 150 / 299 (contexts 452 / 539 / 688); rows 0 and 1 also equal late.npz, the first 64 steps b32.npz;
    the sampling arguments change nothing (reference wrapper.py:220-232 never removes the arg-max); a long run extends a short one."""
    a1, a2, ids = synth.make_batch(32)
    t300, lens, n, _ = engine.generate(a1, a2, ids, max_len=300, top_p=0.8, temperature=1.0, stop_id=0, ignore_stop=True)
    assert t300.shape == (32, 300) and n == 300 and (t300 >= 0).all() and (t300 < 49152).all()
    late = np.load(os.path.join(golden_dir, "late.npz"))
    assert np.array_equal(t300[:2], late["tokens"])
    b32 = np.load(os.path.join(golden_dir, "b32.npz"))
    assert np.array_equal(t300[:, : b32["tokens"].shape[1]], b32["tokens"])
    long_path = os.path.join(golden_dir, "b32long.npz")
    assert os.path.exists(long_path), "tests/golden/b32long.npz is part of the tree: configs[2] is pinned to it"
    gl = np.load(long_path)
    # 9600 greedy decisions; the reference's own top-2 logit gap is below twice the 3e-3 logit tolerance at NINE of them (counted
    # and named in tests/test_oracle_golden.py::test_reference_near_ties_are_counted; the smallest: 8.4e-5 at (row 10, step 153),
    # 2.1e-4 at (row 19, step 243)), where an fp32 implementation that differs from ATen's summation order may legitimately take
    # the other token -- and then continues on another sequence.  Every row must equal the reference up to its first departure,
    # a departure may only happen AT one of those nine decisions, and the departures of each precision mode are exactly the
    # ones recorded here (an engine change that moves them has to be looked at and recorded).
    near = {(int(r), int(s)) for s, r in np.argwhere(gl["top2_gap"] < 6e-3)}
    left = []
    for r in range(32):
        d = np.flatnonzero(t300[r] != gl["tokens"][r])
        if d.size:
            left.append((r, int(d[0])))
    mode = engine.precision
    print(f"[{mode}] configs[2] per-rank run: {9600 - sum(300 - st for _, st in left)} of 9600 tokens equal the reference's; rows that "
          f"left it (row, step, reference gap): {[(r, st, float(gl['top2_gap'][st, r])) for r, st in left]}")
    assert set(left) <= near, f"[{mode}] a row leaves the reference's 300-step run away from a near-tie: {left}"
    assert set(left) == _B32LONG_DEPARTURES[mode], f"[{mode}] departures from the reference's run moved: {left}"
    # teacher-forced logits late in the run: prefill of [prefix | embed(reference tokens)] up to the kept step
    pre = engine.prefix(a1[:8], a2[:8], ids[:8])
    sd_embed = synth.make_state_dict(0)[spec.LM + "model.embed_tokens.weight"]
    sub = torch.from_numpy(gl["sub_vocab"])
    for k, st in enumerate(gl["keep_steps"].tolist()):
        ext = torch.cat((pre.cpu(), sd_embed[torch.from_numpy(gl["tokens"][:8, :st]).long()]), 1)
        lg = engine.lm_prefill(ext, reserve=2)
        _close(lg[:, sub], gl["logits_sub"][k][:8], rel=0, atol=3e-3, name=f"rows 0..7 at step {st} (context {389 + st})")
        assert lg.argmax(-1).cpu().tolist() == gl["tokens"][:8, st].tolist()
    t64, *_ = engine.generate(a1[:4], a2[:4], ids[:4], max_len=64, top_p=0.3, temperature=0.7, stop_id=0, ignore_stop=True)
    assert np.array_equal(t64, t300[:4, :64])
    # reference stop rule at this length: stop id := a token row 2 first produces late in the run
    row = t300[2]
    k = next(i for i in range(200, 300) if row[i] not in row[:i])
    ts, lens, n, _ = engine.generate(a1[2:3], a2[2:3], ids[2:3], max_len=300, stop_id=int(row[k]))
    assert int(lens[0]) == k and n >= k + 1 and np.array_equal(ts[0, : k + 1], row[: k + 1])


def test_f32_and_f32x3_agree_over_the_300_step_run(engine_f32, synth_sd, golden_dir):
    """The two precision modes against EACH OTHER on BASELINE configs[2]'s per-rank run (32 rows x 300 steps): every row that
    stays on the reference (31 of 32, see the departures table above) is token-identical between the modes for all 300 steps,
    and row 10 -- which both modes take off the reference at its 8.4e-5 near-tie of step 153 -- is identical up to there; after
    it the two modes may follow different sequences (they are different fp32 summation orders on a sequence the reference never
    produced), which is reported, not asserted."""
    from mellow_amd.engine import Engine
    e3 = Engine(device=0, precision="f32x3")
    e3.load_state_dict(synth_sd)
    a1, a2, ids = synth.make_batch(32)
    t0, *_ = engine_f32.generate(a1, a2, ids, max_len=300, stop_id=0, ignore_stop=True)
    t3, *_ = e3.generate(a1, a2, ids, max_len=300, stop_id=0, ignore_stop=True)
    e3.close()
    gl = np.load(os.path.join(golden_dir, "b32long.npz"))
    for r in range(32):
        d = np.flatnonzero(t0[r] != t3[r])
        if r == 10:
            assert d.size == 0 or int(d[0]) >= 153, (r, d[:4])
            print("row 10 after its departure from the reference: the modes", "agree" if d.size == 0 else f"part at step {int(d[0])}")
        else:
            assert d.size == 0, (r, int(d[0]))
            assert np.array_equal(t0[r], gl["tokens"][r])


def test_config4_shape_30s_clips_max_len_128(engine, golden_dir):
    """BASELINE configs[3] at its full size: batch 64, 2 x 30 s clips (7 encoder crops per clip = 896 crops), max_len=128.
    Rows 0 and 1 are pinned to the REFERENCE itself (tests/golden/cfg3.npz: the imported reference's `generate_prefix_inference`
    -- the 7-crop long path of htsat.py:908-936 -- and 16 steps of its unmodified `_generate_batch` on the same two examples):
    tokens equal, prefix within the encoder tolerance, teacher-forced logits within 3e-3.  A row's tokens do not depend on the batch around it (rows 4 and 63 alone give the same 128
    tokens, although a one-row-block batch runs the fused down + q/k/v launch and the 64-row batch the five-launch layer)."""
    g = np.load(os.path.join(golden_dir, "cfg3.npz"))
    B, L = 64, 128
    assert int(g["n_samples"]) == 30 * spec.SAMPLE_RATE and int(g["rows"]) == 2
    a1, a2, ids = synth.make_batch(B, n_samples=30 * spec.SAMPLE_RATE)
    t, lens, n, _ = engine.generate(a1, a2, ids, max_len=L, stop_id=0, ignore_stop=True)
    assert t.shape == (B, L) and n == L
    steps = int(g["steps"])
    bad = np.argwhere(t[:2, :steps] != g["tokens"])
    assert bad.size == 0, f"first divergence from the reference at (row, step) {bad[0].tolist()}"
    for r in (4, 63):
        t1, *_ = engine.generate(a1[r:r + 1], a2[r:r + 1], ids[r:r + 1], max_len=L, stop_id=0, ignore_stop=True)
        assert np.array_equal(t1[0], t[r]), r
    pre = engine.prefix(a1[:2], a2[:2], ids[:2])
    _close(pre[:, ::3, ::5], g["prefix_sub"], name="30 s prefix of rows 0, 1 (sub-sampled) vs the reference")
    sub = torch.from_numpy(g["sub_vocab"])
    logits = engine.lm_prefill(pre, reserve=steps)
    for i in range(steps):
        if i:
            logits = engine.lm_decode_step(g["tokens"][:, i - 1])
        _close(logits[:, sub], g["logits_sub"][i], rel=0, atol=3e-3, name=f"30 s clips: logits at step {i}")
        _close(logits.max(-1).values, g["logits_max"][i], rel=0, atol=3e-3, name=f"30 s clips: max logit at step {i}")


def test_fused_and_five_launch_decode_layers_agree(engine_f32, synth_sd, monkeypatch, golden_dir):
    """The decode layer runs as 4 launches (the down projection of a layer and the q/k/v projection of the next one in one kernel,
    on the weight W'Wd composed at load time) or, with the engine option decode_fuse = 0, as the 5 launches of round 2.  Both must give the
    reference's tokens (the fused form is what every other test exercises); their last-position logits differ only by fp32
    summation-order noise.  B = 2 for 40 steps, and B = 33 (two row blocks, the second with one row)."""
    from mellow_amd.engine import Engine
    e5 = Engine(device=0, precision="f32", options={"decode_fuse": 0})
    e5.load_state_dict(synth_sd)
    try:
        g = np.load(os.path.join(golden_dir, "late.npz"))
        a1, a2, ids = synth.make_batch(2)
        t5, *_ = e5.generate(a1, a2, ids, max_len=40, stop_id=0, ignore_stop=True)
        t4, *_ = engine_f32.generate(a1, a2, ids, max_len=40, stop_id=0, ignore_stop=True)
        assert np.array_equal(t5, g["tokens"][:, :40]) and np.array_equal(t4, t5)
        prefix = engine_f32.prefix(a1, a2, ids)
        l4 = engine_f32.lm_prefill(prefix, reserve=4)
        l5 = e5.lm_prefill(prefix, reserve=4)
        for step in range(3):
            _close(l4, l5, rel=0, atol=1e-3, name=f"fused vs five-launch logits, step {step}")
            tok = l5.argmax(-1).to(torch.int32)
            l4, l5 = engine_f32.lm_decode_step(tok), e5.lm_decode_step(tok)
        b1, b2, bi = synth.make_batch(33)
        u5, *_ = e5.generate(b1, b2, bi, max_len=6, stop_id=0, ignore_stop=True)
        u4, *_ = engine_f32.generate(b1, b2, bi, max_len=6, stop_id=0, ignore_stop=True)
        assert np.array_equal(u4, u5)
    finally:
        e5.close()


def test_split_prefill_is_bit_identical_to_one_chain(synth_sd, monkeypatch):
    """f32x3 mode runs the LM prefill as two independent half-batches on two streams (engine_lm.cpp run_prefill; 1 / 3 / 4 parts by
    the engine option prefill_split).  A row's arithmetic does not depend on which rows share its launch, so logits and tokens must be
    BIT-identical to the one-chain form, for batches that split unevenly (3, 5), not at all (1) and into four parts (9)."""
    from mellow_amd.engine import Engine
    engs = {}
    for parts in ("1", "2", "4"):
        engs[parts] = Engine(device=0, precision="f32x3", options={"prefill_split": int(parts)})
        engs[parts].load_state_dict(synth_sd)
    for B in (1, 3, 5, 9):
        a1, a2, ids = synth.make_batch(B)
        pre = engs["1"].prefix(a1, a2, ids)
        ref = engs["1"].lm_prefill(pre, reserve=4)
        tref, *_ = engs["1"].generate(a1, a2, ids, max_len=6, stop_id=0, ignore_stop=True)
        for parts in ("2", "4"):
            assert torch.equal(engs[parts].lm_prefill(pre, reserve=4), ref), (B, parts)
            t, *_ = engs[parts].generate(a1, a2, ids, max_len=6, stop_id=0, ignore_stop=True)
            assert np.array_equal(t, tref), (B, parts)
    for e in engs.values():
        e.close()


def test_norm_free_prefill_agrees_with_the_two_launch_form(synth_sd, monkeypatch, golden_dir):
    """f32x3 LM prefill without RMSNorm launches (round 4, engine_lm.cpp run_prefill): the o_proj / down GEMMs emit their output
    pre-split together with its sum-of-squares partials, the q/k/v and gate/up GEMMs run on norm-folded weights and scale their
    accumulators by the row statistic.  Against the form with a normalisation launch in front of each of those GEMMs
    (engine option prefill_fuse_norm = 0): same tokens, last-position and all-position logits within a third of the 3e-3 the mode is held
    to against the reference (both forms pass the reference tests on their own: the `engine` fixture runs the default)."""
    from mellow_amd.engine import Engine
    e2 = Engine(device=0, precision="f32x3", options={"prefill_fuse_norm": 0})
    e2.load_state_dict(synth_sd)
    e1 = Engine(device=0, precision="f32x3")
    e1.load_state_dict(synth_sd)
    try:
        for B in (1, 3, 32):
            a1, a2, ids = synth.make_batch(B)
            pre = e2.prefix(a1, a2, ids)
            l2, l1 = e2.lm_prefill(pre, reserve=4), e1.lm_prefill(pre, reserve=4)
            _close(l1, l2, rel=0, atol=1e-3, name=f"norm-free prefill logits, B = {B}")
            assert l1.argmax(-1).tolist() == l2.argmax(-1).tolist()
            t2, *_ = e2.generate(a1, a2, ids, max_len=12, stop_id=0, ignore_stop=True)
            t1, *_ = e1.generate(a1, a2, ids, max_len=12, stop_id=0, ignore_stop=True)
            assert np.array_equal(t1, t2), B
        f = np.load(os.path.join(golden_dir, "forward.npz"))
        a1, a2, ids = synth.make_batch(2)
        ans = torch.from_numpy(f["answer_ids"])
        _close(e1.forward(a1, a2, ids, ans, from_pos=int(f["from_pos"])), e2.forward(a1, a2, ids, ans, from_pos=int(f["from_pos"])),
               rel=0, atol=1e-3, name="all-position logits (training-time forward)")
    finally:
        e1.close(); e2.close()


def test_encoder_presplit_handover_and_splitk_agree_with_the_plain_form(synth_sd, monkeypatch):
    """f32x3 encoder, round 4 (engine_encoder.cpp run_encoder): in Swin stages 2-3 the LayerNorms, the window attention and the
    GELU epilogue of fc1 hand their output over pre-split (APB) and qkv / proj / fc1 / fc2 run on the LDS-DMA kernel; in stage 0
    the LayerNorms hand over pre-split and the K = 96 GEMMs qkv / fc1 run on the weight-stationary persistent kernel
    (gemm_x3w_kernel; B = 32 here is what reaches its M >= 8192 rows); launches of <= 256 output tiles (stage 3 fc2, the
    token-semantic conv, small batches) are split along K with a fixed summation order.  Against the plain form (engine options enc_apb = 0, splitk = 0: fp32 hand-over, register-staged kernel, no
    split): the encoder output within 2e-5 of its maximum (both forms pass the oracle / reference taps on their own: the
    `engine` fixture runs the default), the same tokens; and every single switch on its own as well."""
    from mellow_amd.engine import Engine

    def make(options):
        e = Engine(device=0, precision="f32x3", options=options)
        e.load_state_dict(synth_sd)
        return e

    plain = make({"enc_apb": 0, "splitk": 0})
    forms = {"default": make({}), "all stages": make({"enc_apb": 0xFF}), "no split-K": make({"splitk": 0}),
             "split-K only": make({"enc_apb": 0}), "no proj hand-over": make({"enc_apb": 0x0E}),
             "stage 0 without the weight-stationary kernel": make({"enc_apb": 0xCC}),
             "stage 0 pre-split on the tile kernels": make({"x3w": 0})}
    try:
        for B in (1, 3, 32):
            a1, a2, ids = synth.make_batch(B)
            wav = np.concatenate([np.asarray(a1), np.asarray(a2)], 0)
            want = plain.encode(wav).cpu().numpy()
            tref, *_ = plain.generate(a1, a2, ids, max_len=10, stop_id=0, ignore_stop=True)
            for name, e in forms.items():
                got = e.encode(wav).cpu().numpy()
                assert np.isfinite(got).all(), (name, B)
                err = np.abs(got - want).max() / np.abs(want).max()
                assert err < 2e-5, (name, B, err)
                t, *_ = e.generate(a1, a2, ids, max_len=10, stop_id=0, ignore_stop=True)
                assert np.array_equal(t, tref), (name, B)
                again = e.encode(wav).cpu().numpy()
                assert np.array_equal(again, got), (name, B, "not deterministic")
    finally:
        plain.close()
        for e in forms.values():
            e.close()


def test_fork_needs_a_loaded_engine_and_shares_its_answers(engine_f32):
    from mellow_amd.engine import Engine, EngineError
    raw = Engine(device=0, precision="f32")
    with pytest.raises(EngineError, match="fork needs"):
        raw.fork()
    raw.close()
    child = engine_f32.fork()
    a1, a2, ids = synth.make_batch(2)
    want, *_ = engine_f32.generate(a1, a2, ids, max_len=5, stop_id=0, ignore_stop=True)
    got, *_ = child.generate(a1, a2, ids, max_len=5, stop_id=0, ignore_stop=True)
    assert np.array_equal(got, want)
    child.close()
    again, *_ = engine_f32.generate(a1, a2, ids, max_len=5, stop_id=0, ignore_stop=True)      # the parent outlives its fork
    assert np.array_equal(again, want)


def test_pipelined_contexts_give_identical_tokens(engine_f32, synth_sd):
    """mellow_amd.serve.EnginePool: three contexts on one GPU sharing one weight copy, batches in flight concurrently == one engine,
    batch by batch."""
    from mellow_amd.serve import EnginePool
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    pool = EnginePool(synth_sd, n_contexts=3, device=0)
    batches = [synth.make_batch(3, first=3 * i) for i in range(6)]
    got = pool.generate_many(batches, max_len=6, stop_id=0, ignore_stop=True)
    free1, _ = torch.cuda.mem_get_info(0)
    # the contexts share ONE weight arena (mellow_engine_fork; 3.4 GB reserved) + per-context workspaces (measured 6.1 GB in
    # all): three separate engines would hold > 10 GB in arenas alone
    assert free0 - free1 < 8e9, (free0 - free1) / 1e9
    assert pool.engines[1]._parent is pool.engines[0] and pool.engines[2]._parent is pool.engines[0]
    pool.close()
    for (a1, a2, ids), res in zip(batches, got):
        want, *_ = engine_f32.generate(a1, a2, ids, max_len=6, stop_id=0, ignore_stop=True)
        assert np.array_equal(res[0], want)


# ---- BASELINE config 5: fp8 (e4m3) GEMM mode --------------------------------------------------------------------
def _quant_rows_e4m3(x):
    amax = x.abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = torch.where(amax > 0, 448.0 / amax, torch.zeros_like(amax))
    return (x * inv).to(torch.float8_e4m3fn).to(torch.float32), scale


def _quant_mx8(x):
    """MXFP8 as the engine's producers emit it (mellow_amd/csrc/common.h: amx_store_block): e4m3 elements and, per 32 consecutive
    k of a row, the smallest power-of-two scale with amax / scale <= 448 (no element clips; an all-zero block takes 2^0).
    Returns the dequantised values (exact in fp32)."""
    M, K = x.shape
    Kp = (K + 31) // 32 * 32
    xb = torch.zeros(M, Kp, dtype=torch.float32)
    xb[:, :K] = x
    xb = xb.view(M, Kp // 32, 32)
    amax = xb.abs().amax(-1, keepdim=True)
    mant, ex = torch.frexp(amax / 448.0)                       # amax / 448 = mant * 2^ex, mant in [0.5, 1)
    e = torch.where(mant > 0.5, ex, ex - 1)                    # ceil(log2(amax / 448))
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    q = (xb / scale).to(torch.float8_e4m3fn).to(torch.float32)
    return (q * scale).view(M, Kp)[:, :K]


def test_fp8_gemm_matches_quantised_emulation(engine_f32):
    """The fp8 GEMM (round 6: v_mfma_scale_f32_32x32x64_f8f6f4, activations MXFP8 with one E8M0 scale per 32 k, weights e4m3 per
    output channel) == exact products of the SAME quantised operands.  Tolerance: the accumulation of the fp8 matrix pipe (measured
    with tools/microbench/mx8_semantics.hip: ~4e-5 of the largest element, coarser than an fp32 fmaf chain) -> 1e-4 of max for all
    but a few elements, plus the rare element whose scaled value sits on a rounding tie and lands one e4m3 step apart (bounded by
    2e-3 of max); the quantisation itself costs percents vs the exact product.  K = 96 and K = 224 exercise the zero-padded k64
    tail, M = 70 / 389 the ragged last row panel."""
    torch.manual_seed(1)
    for M, N, K in ((70, 36, 64), (389, 576, 576), (300, 960, 1536), (4097, 288, 96), (129, 128, 224)):
        A = torch.randn(M, K) * (0.2 + 3 * torch.rand(M, 1))
        A[:, : K // 2] *= 30.0                                         # blocks of very different magnitude inside one row
        W = torch.randn(N, K) * 0.05 * (1 + torch.rand(N, 1))
        A[3] = 0.0                                                     # an all-zero row must quantise to zeros
        got, _ = engine_f32.debug_gemm_fp8(A, W)
        Aq = _quant_mx8(A)
        Wq, sw = _quant_rows_e4m3(W)
        ref = (Aq.double() @ Wq.double().T) * sw.double().T
        exact = A.double() @ W.double().T
        scale = float(ref.abs().max())
        d = (got.double() - ref).abs()
        assert torch.isfinite(got).all()
        assert float(d.max()) <= 2e-3 * scale, (M, N, K, float(d.max()), scale)
        assert float((d > 1e-4 * scale).double().mean()) < 1e-3, (M, N, K)          # almost every element is accumulation noise only
        assert float(got[3].abs().max()) == 0.0
        assert float((ref - exact).abs().max()) > 2e-3 * scale            # sanity: the emulation really is quantised
        # block scaling: a row's small-magnitude half keeps its own precision (a per-row scale would lose it to the 30x larger half)
        assert float((Aq[:, K // 2:] - A[:, K // 2:]).abs().max()) <= 0.07 * float(A[:, K // 2:].abs().max())


def test_fp8_decode_weights_equal_their_dequantised_fp32_form(synth_sd, golden_dir):
    """BASELINE config 5, decode half: the five decode GEMM kernels read e4m3 weights (one scale per packed weight row, values
    widened in registers, fp32 activations and accumulation).  Isolation: a checkpoint whose LM matrices are ALREADY e4m3-
    representable per output row (quantise -> dequantise in torch; RMSNorm weights 1 so that folding them into the decode
    operands changes nothing) goes (a) into an fp8 engine with its e4m3 PREFILL switched off (engine option fp8_prefill = 0) and (b) into
    a plain fp32 engine.  Re-quantising is the identity, so both must produce the same decode-step logits up to fp32 rounding
    (the scale is applied after the reduction instead of per weight), over 6 teacher-forced steps, and the same tokens."""
    from mellow_amd.engine import Engine
    sd = dict(synth_sd)
    lm_mats = [k for k in sd if k.startswith("caption_decoder.lm.") and k.endswith(".weight") and sd[k].dim() == 2]
    assert len(lm_mats) == 30 * 7 + 2                       # q k v o gate up down per layer + embed_tokens + its tied lm_head
    for k in lm_mats:
        q, sc = _quant_rows_e4m3(sd[k].float())
        sd[k] = (q * sc).contiguous()
    for k in sd:
        if k.endswith("input_layernorm.weight") or k.endswith("post_attention_layernorm.weight"):
            sd[k] = torch.ones_like(sd[k])
    # fp32 activations (the weights are the only quantised operand here), fp32 K/V pages (the mode's bf16 shadow pages have their
    # own test below), and no fused launch: it multiplies by W' Wd, which is not an e4m3 matrix
    e8 = Engine(device=0, precision="fp8", options={"fp8_prefill": 0, "fp8_decode_act": 0, "fp8_kv16": 0, "decode_fuse": 0})
    e8.load_state_dict(sd)
    e32 = Engine(device=0, precision="f32")
    e32.load_state_dict(sd)
    a1, a2, ids = synth.make_batch(3)
    pre = e32.prefix(a1, a2, ids)
    _close(e8.prefix(a1, a2, ids), pre, rel=1e-6, name="prefix (no e4m3 GEMM in this engine's encoder)")
    l32 = e32.lm_prefill(pre, reserve=8)
    l8 = e8.lm_prefill(pre, reserve=8)
    for i in range(6):
        scale = float(l32.abs().max())
        _close(l8, l32, rel=0, atol=2e-5 * scale, name=f"e4m3-weight decode logits, step {i}")
        tok = l32.argmax(-1)
        assert torch.equal(l8.argmax(-1), tok)
        l32 = e32.lm_decode_step(tok)
        l8 = e8.lm_decode_step(tok)
    # and the quantisation is real: against the UN-quantised checkpoint the same engine differs at the percent level
    e0 = Engine(device=0, precision="f32")
    e0.load_state_dict(synth_sd)
    l0 = e0.lm_prefill(e0.prefix(a1, a2, ids), reserve=2)
    e8b = Engine(device=0, precision="fp8", options={"fp8_prefill": 0})
    e8b.load_state_dict(synth_sd)
    l8b = e8b.lm_prefill(e8b.prefix(a1, a2, ids), reserve=2)
    rel = float((l8b - l0).pow(2).mean().sqrt() / l0.pow(2).mean().sqrt())
    assert 1e-3 < rel < 0.2, rel            # only the LAST layer's tail + lm_head run on e4m3 weights in a prefill call
    for e in (e8, e32, e0, e8b):
        e.close()


def test_fp8_mode_bf16_kv_shadow_pages(synth_sd):
    """fp8 mode: the decode step reads and extends a bf16 SHADOW of the K/V pages -- half the bytes of the step's
    largest stream (at B = 128 the step reads 2.5 GB of fp32 K/V against 0.13 GB of e4m3 weights).  Against the same engine
    on fp32 pages (engine option fp8_kv16 = 0) the teacher-forced decode logits stay well inside the fp8 mode's own distance from the
    fp32 engine (0.26 relative rms): the e4m3 activation rounding amplifies the 2^-9 perturbation of K and V to a measured
    8e-2 relative rms (bound 0.25); finite and deterministic, at B = 3 and B = 40 (two row blocks).  Token agreement with the
    fp32 engine is the same with either page format (profiles/r05_fp8_agreement*.txt: position-wise 0.705 / 0.680)."""
    from mellow_amd.engine import Engine
    ea = Engine(device=0, precision="fp8")
    eb = Engine(device=0, precision="fp8", options={"fp8_kv16": 0})
    ea.load_state_dict(synth_sd)
    eb.load_state_dict(synth_sd)
    for B in (3, 40):
        a1, a2, ids = synth.make_batch(B)
        pre = eb.prefix(a1, a2, ids)
        la, lb = ea.lm_prefill(pre, reserve=8), eb.lm_prefill(pre, reserve=8)
        for i in range(6):
            rel = float((la - lb).pow(2).mean().sqrt() / lb.pow(2).mean().sqrt())
            assert torch.isfinite(la).all() and rel < 0.25, (B, i, rel)
            if i > 0:
                assert rel > 1e-6, (B, i, rel)          # the shadow pages are really in use
            tok = lb.argmax(-1)
            la, lb = ea.lm_decode_step(tok), eb.lm_decode_step(tok)
    ea.close()
    eb.close()


def _e4m3_grid(shape, gen):
    """Random values that ARE e4m3 numbers (normal range, both signs)."""
    x = torch.randn(shape, generator=gen).clamp(-3, 3) * 100.0
    return x.to(torch.float8_e4m3fn).to(torch.float32)


def test_fp8_decode_activation_quantisation_is_exact_on_representable_rows(synth_sd):
    """The activation half of the fp8 decode kernels (v_mfma_f32_32x32x16_fp8_fp8 / 16x16x32: e4m3 weights AND activations,
    one activation scale per batch row and k-slice of a wave = amax / 448), pinned through the lm_head kernel
    (`mellow_debug_dec_head`): rows whose every 72-column slice is (an e4m3 number) x 2^e with slice amax 448 x 2^e quantise
    without loss, so the fp8-pipe result must equal the same kernel on fp32 activations up to fp32 summation order -- which
    also proves that weight bytes and activation bytes meet at the same k inside the instruction.  A generic row then differs
    at the e4m3 level (3-bit mantissa), not more."""
    from mellow_amd.engine import Engine
    e8 = Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    gen = torch.Generator().manual_seed(5)
    for B in (3, 32, 40):
        q = _e4m3_grid((B, 8, 72), gen)
        q[:, :, 0] = 448.0 * torch.where(torch.rand((B, 8), generator=gen) < 0.5, -1.0, 1.0)      # every slice reaches the format's maximum
        expo = torch.randint(-12, 6, (B, 8, 1), generator=gen).float()
        x = (q * torch.exp2(expo)).reshape(B, 576)
        x[0, 72:144] = 0.0                                  # an all-zero slice
        ref = e8.debug_dec_head(x, act_fp8=False)
        got = e8.debug_dec_head(x, act_fp8=True)
        scale = float(ref.abs().max())
        # (the fp8 instruction sums its 16 products with fewer guard bits than an fp32 FMA chain: measured 1.6e-5 of max,
        #  the same class as the prefill GEMM's 1e-4 bound above; a mis-assigned k would be O(1))
        _close(got, ref, rel=0, atol=1e-4 * scale, name=f"fp8-pipe lm_head on representable rows, B={B}")
        assert torch.equal(got.argmax(-1), ref.argmax(-1))
    xg = torch.randn((32, 576), generator=gen)
    ref = e8.debug_dec_head(xg, act_fp8=False)
    got = e8.debug_dec_head(xg, act_fp8=True)
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert 5e-3 < rel < 6e-2, rel                           # e4m3 rounding: 2^-4 / sqrt(3) = 3.6e-2 per element
    e8.close()


def test_fp8_decode_on_the_fp8_pipe_stays_near_the_fp32_activation_form(synth_sd):
    """Whole decode steps, e4m3 weights in both engines, activations fp32 (engine option fp8_decode_act = 0) against e4m3 on the fp8
    matrix pipe (the default of the fp8 mode): five GEMM kernels per layer quantise their inputs, so the logits differ at the
    percent level -- a wrong lane/byte assignment in any of them would give an O(1) difference -- and stay deterministic."""
    from mellow_amd.engine import Engine
    ew = Engine(device=0, precision="fp8", options={"fp8_prefill": 0, "fp8_decode_act": 0})
    ea = Engine(device=0, precision="fp8", options={"fp8_prefill": 0})
    ew.load_state_dict(synth_sd)
    ea.load_state_dict(synth_sd)
    # ... and the fp8 mode's fused launch (down of layer l + q/k/v of layer l+1 on the e4m3 copy of W' Wd, dec_gemv.hip) against
    # the five-launch layer on the same engine settings
    eu = Engine(device=0, precision="fp8", options={"decode_fuse": 0})
    eu.load_state_dict(synth_sd)
    ef = Engine(device=0, precision="fp8")
    ef.load_state_dict(synth_sd)
    for B in (3, 40):
        a1, a2, ids = synth.make_batch(B)
        pre = ew.prefix(a1, a2, ids)
        lw = ew.lm_prefill(pre, reserve=6)
        la = ea.lm_prefill(pre, reserve=6)
        lu = eu.lm_prefill(pre, reserve=6)
        lf = ef.lm_prefill(pre, reserve=6)
        for i in range(4):
            rel = float((la - lw).pow(2).mean().sqrt() / lw.pow(2).mean().sqrt())
            assert torch.isfinite(la).all() and 1e-3 < rel < 0.2, (B, i, rel)
            if i > 0:                      # (a prefill call ends with one decode layer: nothing fused in it)
                relf = float((lf - lu).pow(2).mean().sqrt() / lu.pow(2).mean().sqrt())
                assert torch.isfinite(lf).all() and 1e-4 < relf < 0.2, (B, i, relf)
            tok = lw.argmax(-1)
            lw = ew.lm_decode_step(tok)
            la = ea.lm_decode_step(tok)
            lu = eu.lm_decode_step(tok)
            lf = ef.lm_decode_step(tok)
        la_again = ea.lm_prefill(pre, reserve=6)
        assert torch.equal(la_again, ea.lm_prefill(pre, reserve=6))
    for e in (ew, ea, eu, ef):
        e.close()


def test_fp8_decode_attention_chunks_and_key_splits_agree(synth_sd):
    """bf16-page decode attention (fp8 mode: scores on the matrix pipe, dec_attn.hip at `DA_GM`): a wave walks its keys in chunks of
    one 32-key tile and rescales its running (m, l, o) between chunks, and the key range is cut into two splits at a boundary that
    follows the RESERVED context.  Every benchmarked configuration keeps a split inside one chunk; here the same 389-key prefix is
    decoded with 8 and with 400 reserved positions -- the second puts keys 0..395 into split 0 as TWO chunks per wave (rescale
    path, partly masked second tile) and leaves split 1 with the appended keys only.  Same arithmetic in another summation order;
    in this mode an e4m3 activation rounding downstream turns the 1e-7 into a flipped code here and there, so the logits of the
    teacher-forced steps agree to 1.5e-2 .. 2.6e-2 relative rms (measured; a build of that round with the vector form
    shows the same 1.5e-2 .. 2.6e-2 on the same box: the figure is the mode's, not the kernel's) -- asserted < 6e-2, with both runs
    at the mode's own distance (0.05 .. 0.18) from the fp32-accurate engine on the structured checkpoint.  A wrong rescale or mask
    would put O(1) errors into every row."""
    from mellow_amd.engine import Engine
    sds = synth.make_state_dict(0, structured=True)
    e8, e32 = Engine(device=0, precision="fp8"), Engine(device=0, precision="f32x3")
    e8.load_state_dict(sds); e32.load_state_dict(sds)
    a1, a2, ids = synth.make_batch(8)
    pre = e32.prefix(a1, a2, ids)
    ref = [e32.lm_prefill(pre, reserve=8).clone()]
    for i in range(3):
        ref.append(e32.lm_decode_step(ref[-1].argmax(-1)).clone())
    runs = []
    for reserve in (8, 400):
        out = [e8.lm_prefill(pre, reserve=reserve).clone()]
        for i in range(3):
            out.append(e8.lm_decode_step(ref[i].argmax(-1)).clone())     # teacher-forced with the fp32-accurate tokens
        runs.append(out)
    rr = lambda x, y: float((x - y).pow(2).mean().sqrt() / y.pow(2).mean().sqrt())
    for i in range(4):              # (step 0 = the prompt's last position: it runs through the decode kernels too)
        d = rr(runs[1][i], runs[0][i])
        assert torch.isfinite(runs[1][i]).all() and d < 6e-2, (i, d)
        assert rr(runs[0][i], ref[i]) < 0.35 and rr(runs[1][i], ref[i]) < 0.35, (i, rr(runs[0][i], ref[i]), rr(runs[1][i], ref[i]))
        print(f"step {i}: reserve 400 vs 8 rel rms {d:.2e}; vs f32x3 {rr(runs[0][i], ref[i]):.3f} / {rr(runs[1][i], ref[i]):.3f}")
    e8.close(); e32.close()


def test_fp8_mode_end_to_end(synth_sd, engine_f32, golden_dir):
    """precision="fp8": e4m3 GEMMs in the Swin linears and LM prefill, e4m3 WEIGHTS in the five decode GEMM kernels and the
    lm_head (fp32 activations there); front-end, attentions and norms fp32.  Not bit-exact by design; the test pins (a)
    determinism, (b) bounded error against the fp32 engine, (c) that the fp32 engine is untouched, (d) token agreement with the
    fp32 engine where that number means something.  On the i.i.d.-Gaussian (un-trained) synthetic checkpoint a random network
    re-amplifies 3-bit-mantissa noise in every layer: first-token agreement there is a coin flip per row (round 5, per-row scales:
    10 of these 16 rows; round 6, MXFP8 block scales: 7 of 16 -- both inside the binomial noise of p ~ 0.5), so only a loose floor
    is asserted on it; the meaningful figure is taken on the STRUCTURED checkpoint (decaying singular spectra, synth.py), where
    round 6 measures first-token 0.84 / position-wise 0.90 over 32 x 64 (round 5: 0.72 / 0.71); see DESIGN.md 6b."""
    from mellow_amd.engine import Engine
    e8 = Engine(device=0, precision="fp8")
    e8.load_state_dict(synth_sd)
    B = 16
    a1, a2, ids = synth.make_batch(B)
    p32 = engine_f32.prefix(a1, a2, ids)
    p8 = e8.prefix(a1, a2, ids)
    rel = float((p8 - p32).pow(2).mean().sqrt() / p32.pow(2).mean().sqrt())
    # error model: one e4m3 GEMM costs ~4e-2 of max (3-bit mantissa, per-row / per-channel scales); the encoder chains ~50 of
    # them with LayerNorms in between and lands at 4.9e-2 rel-rms on this checkpoint: bounds at 1.6x the measured values
    assert torch.isfinite(p8).all() and 1e-3 < rel < 0.08, rel
    l32 = engine_f32.lm_prefill(p32, reserve=2).cpu()
    l8 = e8.lm_prefill(p32, reserve=2).cpu()
    rel_l = float((l8 - l32).pow(2).mean().sqrt() / l32.pow(2).mean().sqrt())
    assert torch.isfinite(l8).all() and 1e-3 < rel_l < 0.27, rel_l       # measured 0.165 (30 layers x 4 fp8 GEMMs)
    t8a, *_ = e8.generate(a1, a2, ids, max_len=8, stop_id=0, ignore_stop=True)
    t8b, *_ = e8.generate(a1, a2, ids, max_len=8, stop_id=0, ignore_stop=True)
    assert np.array_equal(t8a, t8b)                                      # deterministic
    t32, *_ = engine_f32.generate(a1, a2, ids, max_len=8, stop_id=0, ignore_stop=True)
    agree = float((t8a[:, 0] == t32[:, 0]).mean())
    assert agree >= 0.25, agree                                          # i.i.d. checkpoint: noise-dominated (see above); chance is 1/49152
    # (d) the structured checkpoint: 32 rows x 16 tokens against the fp32-accurate default engine
    sds = synth.make_state_dict(0, structured=True)
    es8, es32 = Engine(device=0, precision="fp8"), Engine(device=0, precision="f32x3")
    es8.load_state_dict(sds); es32.load_state_dict(sds)
    s1, s2, sid = synth.make_batch(32)
    ts8, *_ = es8.generate(s1, s2, sid, max_len=16, stop_id=0, ignore_stop=True)
    ts32, *_ = es32.generate(s1, s2, sid, max_len=16, stop_id=0, ignore_stop=True)
    first, posw = float((ts8[:, 0] == ts32[:, 0]).mean()), float((ts8 == ts32).mean())
    assert first >= 0.75 and posw >= 0.70, (first, posw)                 # measured 0.84 / 0.78 over 16 tokens (0.84 / 0.90 over 64: tools/fp8_agreement.py)
    es8.close(); es32.close()
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    assert np.array_equal(t32[:2], g["tokens"][:, :8])                   # the exact path still matches the reference goldens
    # config 5's batch (128, max_len 64): every quantisation scale belongs to one batch row, so the first 16 rows of the big
    # batch must equal the small batch exactly -- for the same max_len: the reserved context fixes the key split of the decode
    # attention, a different split is a different fp32 summation order, and an e4m3 rounding downstream can turn a 1e-7
    # difference into a different token
    a1b, a2b, idsb = synth.make_batch(128)
    t128, _, n128, _ = e8.generate(a1b, a2b, idsb, max_len=64, stop_id=0, ignore_stop=True)
    assert t128.shape == (128, 64) and n128 == 64 and (t128 >= 0).all() and (t128 < 49152).all()
    t16, *_ = e8.generate(a1, a2, ids, max_len=64, stop_id=0, ignore_stop=True)
    assert np.array_equal(t128[:16], t16)
    e8.close()


def test_fp8_mode_bf16_prefill_attention_stays_near_the_exact_one(synth_sd):
    """fp8 mode, round 6: the LM prefill attention runs on operands rounded ONCE to bf16 (8 MFMAs per 32 x 32 tile instead of the 48
    of the exact 3-way split; engine option fp8_attn_bf16 = 0 keeps the split).  On the SAME prefix the prefill logits of the two
    forms differ by what bf16 rounding of q / k / p / v costs after 29 layers of e4m3 GEMMs -- well inside the mode's own distance
    from the fp32 engine (0.17-0.23 relative rms); a wrong key / lane assignment in the NP = 1 plumbing would be O(1).  Determinism
    and the two row-count regimes (one chain, two parts) included."""
    from mellow_amd.engine import Engine
    eb, ex = Engine(device=0, precision="fp8"), Engine(device=0, precision="fp8", options={"fp8_attn_bf16": 0})
    eb.load_state_dict(synth_sd); ex.load_state_dict(synth_sd)
    assert eb.describe()["non_default"] == [] and ex.describe()["non_default"] == ["fp8_attn_bf16"]
    for B in (1, 2, 33):
        a1, a2, ids = synth.make_batch(B)
        pre = ex.prefix(a1, a2, ids)
        pb = eb.prefix(a1, a2, ids)          # (the option also stores the Swin blocks' q / k / v as bf16 rows: the encoder moves by bf16 rounding
        rel_p = float((pb - pre).pow(2).mean().sqrt() / pre.pow(2).mean().sqrt())      #  amplified by the e4m3 GEMMs behind it, as far as the mode is from fp32)
        assert torch.isfinite(pb).all() and rel_p < 0.08, (B, rel_p)
        lb, lx = eb.lm_prefill(pre, reserve=2), ex.lm_prefill(pre, reserve=2)
        rel_l = float((lb - lx).pow(2).mean().sqrt() / lx.pow(2).mean().sqrt())
        assert torch.isfinite(lb).all() and 1e-5 < rel_l < 0.15, (B, rel_l)
        assert torch.equal(lb, eb.lm_prefill(pre, reserve=2))
    eb.close(); ex.close()


def test_f32x3_mode_is_fp32_accurate(engine_f32, synth_sd, golden_dir):
    """Experimental precision="f32x3": fp32 GEMMs run as exact 3-way bf16 operand splits on the bf16 MFMA pipe.
    (a) one GEMM against an fp64 product: no less accurate than the exact fp32 MFMA kernel (x1.25 slack on max / rms);
    (b) end to end: greedy tokens identical to the fp32 engine and to the reference goldens, logits within the same
        3e-3 tolerance the fp32 path is held to."""
    from mellow_amd.engine import Engine
    torch.manual_seed(2)
    A = torch.randn(389, 576) * (0.2 + 3 * torch.rand(389, 1))
    W = torch.randn(576, 576) * 0.05
    exact = A.double() @ W.double().T
    e_mfma = (engine_f32.debug_gemm_f32(A, W, mode=0)[0].double() - exact).abs()
    for mode in (16, 17):             # the engine's own f32x3 kernels: A split in registers / pre-split + LDS-DMA
        e_x3 = (engine_f32.debug_gemm_f32(A, W, mode=mode)[0].double() - exact).abs()
        assert float(e_x3.max()) <= 1.25 * float(e_mfma.max()) and float(e_x3.pow(2).mean()) <= 1.25 ** 2 * float(e_mfma.pow(2).mean())
    e3 = Engine(device=0, precision="f32x3")
    e3.load_state_dict(synth_sd)
    a1, a2, ids = synth.make_batch(4)
    t3, *_ = e3.generate(a1, a2, ids, max_len=12, stop_id=0, ignore_stop=True)
    t0, *_ = engine_f32.generate(a1, a2, ids, max_len=12, stop_id=0, ignore_stop=True)
    assert np.array_equal(t3, t0)
    g = np.load(os.path.join(golden_dir, "gen.npz"))
    assert np.array_equal(t3[:2], g["tokens"])
    e = np.load(os.path.join(golden_dir, "enc10.npz"))
    prefix = torch.from_numpy(e["prefix"])
    _close(e3.lm_prefill(prefix, reserve=2), engine_f32.lm_prefill(prefix, reserve=2), rel=0, atol=3e-3, name="f32x3 prefill logits")
    e3.close()


@pytest.mark.parametrize("M,N,K", [(389, 576, 576), (12448, 960, 576), (1000, 3072, 576), (517, 576, 1536), (129, 128, 192),
                                   (128, 4, 224), (1, 640, 4608), (4097, 292, 256)])
def test_lds_dma_gemm_is_bit_identical_to_register_staged(engine_f32, M, N, K):
    """`gemm_x3q_kernel` (pre-split activation in fragment order, both operands staged by LDS-DMA with hand-counted waits; mode
    17 of the debug tap) multiplies the same bf16 pieces in the same order as `gemm_x3p_kernel` (mode 16): the results must be
    equal BIT FOR BIT on ragged M (padding rows of the last 128-row panel are never written by the split kernel), N that is not
    a multiple of the 128-column tile, K of 12 .. 288 k16-tiles, and on repetition (a missed wait would show as a flaky row)."""
    torch.manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K) * (0.2 + 3 * torch.rand(M, 1))
    W = torch.randn(N, K) * 0.05 * (1 + torch.rand(N, 1))
    want = engine_f32.debug_gemm_f32(A, W, mode=16)[0]
    for _ in range(3):
        got = engine_f32.debug_gemm_f32(A, W, mode=17)[0]
        assert torch.equal(got, want)
    exact = A.double() @ W.double().T
    assert float((want.double() - exact).abs().max()) <= 2e-6 * float(exact.abs().max()) + 1e-30


def test_degenerate_audio_matches_oracle(engine, synth_sd):
    """Edge inputs of the front-end: digital silence (log-mel floor 1e-10 -> -100 dB everywhere), a full-scale square
    wave, and a single impulse.  The prefix must stay finite and equal the oracle's."""
    from oracle import mellow_oracle as O
    n = 320000
    sil = np.zeros(n, dtype=np.float32)
    sq = np.where((np.arange(n) // 40) % 2 == 0, 1.0, -1.0).astype(np.float32)
    imp = np.zeros(n, dtype=np.float32)
    imp[12345] = 1.0
    a1 = np.stack([sil, sq, imp])
    a2 = np.stack([imp, sil, sq])
    ids = np.stack([synth.make_prompt_ids(i) for i in range(3)])
    got = engine.prefix(a1, a2, ids).cpu()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        want = O.generate_prefix_inference(synth_sd, torch.from_numpy(a1), torch.from_numpy(a2), torch.from_numpy(ids))
    assert torch.isfinite(got).all()
    _close(got, want, rel=5e-4, name="prefix of degenerate audio")


def test_encoder_activations_beyond_4gib(engine, synth_sd, monkeypatch):
    """BASELINE config 4 scale: 98 clips of 30 s = 686 encoder crops, so the stage-0 MLP activation (2.8 M rows x 384 floats)
    is 4.3 GB -- past the reach of a 32-bit byte offset.  Rows are batch-independent, so the last clip (whose rows lie beyond
    the 4 GiB line) and the first must equal the same clips encoded alone, exactly.  (Exactly = with the split-K of the f32x3
    mode's small launches off: its split count follows the row count, so a clip encoded alone sums some dot products in a
    different order -- 1e-6 of the output -- than the same clip inside 98; with it on, the two agree to that.)"""
    from mellow_amd.engine import Engine
    n = 30 * spec.SAMPLE_RATE
    base = [synth.make_clip(i, n) for i in range(4)]
    wav = np.stack([base[i % 4] for i in range(98)])
    big = engine.encode(wav).cpu()
    assert torch.isfinite(big).all()
    exact = engine
    if engine.precision == "f32x3":
        exact = Engine(device=0, precision="f32x3", options={"splitk": 0})
        exact.load_state_dict(synth_sd)
        big_split, big = big, exact.encode(wav).cpu()
        assert float((big_split - big).abs().max()) <= 2e-5 * float(big.abs().max())
    try:
        for idx in (0, 97):
            alone = exact.encode(wav[idx:idx + 1]).cpu()
            assert torch.equal(big[idx], alone[0]), idx
            if exact is not engine:
                split = engine.encode(wav[idx:idx + 1]).cpu()
                assert float((split[0] - big[idx]).abs().max()) <= 2e-5 * float(big[idx].abs().max()), idx
    finally:
        if exact is not engine:
            exact.close()


def test_device_resampler_matches_host_twin(engine_f32):
    """mellow_resample (A0 on the device) == mellow_amd.audio.resample (the host form): 44.1 kHz -> 32 kHz and 48 kHz -> 32 kHz,
    odd lengths, two clips at once.  Tolerance: fp32 summation order of a 459-tap dot product.  BOTH are checked against the
    independent fp64 oracle (test_device_resampler_against_the_independent_fp64_oracle, tests/test_host_cpu.py); the closed-form
    properties of the filter are checked in test_device_resampler_closed_form."""
    from mellow_amd import audio
    rng = np.random.default_rng(9)
    for sr, n in ((44100, 403604), (48000, 12345), (16000, 4000), (22050, 1)):
        x = torch.from_numpy((rng.standard_normal((2, n)) * 0.3).astype(np.float32))
        want = audio.resample(x, sr, 32000)
        got = engine_f32.resample(x, sr, 32000).cpu()
        assert got.shape == want.shape, (sr, n, got.shape, want.shape)
        assert float((got - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max())), (sr, n)


def test_device_resampler_against_the_independent_fp64_oracle(engine_f32, golden_dir):
    """f1 on the device: `mellow_resample` against oracle/resample_oracle.py (fp64 per-output-sample windowed-sinc sums of
    torchaudio's published algorithm, shares nothing with the product) on the reference's own fixture clips (both edges of
    resource/1.wav and 2.wav @ 44.1 kHz) and on 48 / 22.05 / 16 / 8 kHz noise.  Tolerance: the fp64-derived per-sample bound
    (taps + 2) * 2^-24 * sum|x||h|, and 2e-6 of the peak."""
    from oracle import resample_oracle as R
    g = np.load(os.path.join(golden_dir, "example.npz"))
    cases = []
    for k in ("pcm1", "pcm2"):
        w = g[k].astype(np.float32) / 32768.0
        cases += [(k + "_head", 44100, w[None, :60000]), (k + "_tail", 44100, w[None, -45000:])]
    rng = np.random.default_rng(9)
    for sr, n in ((48000, 12345), (22050, 7777), (16000, 4000), (22050, 1), (8000, 333)):
        cases.append((f"noise_{sr}_{n}", sr, (rng.standard_normal((2, n)) * 0.3).astype(np.float32)))
    for name, sr, x in cases:
        want, bound = R.resample(x, sr, 32000, return_bound=True)
        got = engine_f32.resample(torch.from_numpy(x), sr, 32000).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        d = np.abs(got - want)
        assert (d <= R.fp32_tolerance(bound, sr, 32000)).all(), (name, float(d.max()))
        assert d.max() <= 2e-6 * max(1.0, float(np.abs(want).max())), (name, float(d.max()))


def test_device_resampler_closed_form(engine_f32):
    """Properties any sinc-Hann resampler with torchaudio's defaults (width 6, rolloff 0.99) must have, independent of the
    host twin: output length ceil(new*n/orig) for the reference's own fixture lengths (resource/1.wav: 403,604 @ 44.1 kHz ->
    292,865), DC gain 1, an in-band tone keeps amplitude and frequency, a tone above the new Nyquist is rejected."""
    for sr, n, want in ((44100, 403604, 292865), (44100, 441, 320), (48000, 3, 2), (16000, 5, 10)):
        assert engine_f32.resample(torch.zeros(1, n), sr, 32000).shape == (1, want), (sr, n)
    sr, n = 44100, 44100
    dc = engine_f32.resample(torch.full((1, n), 0.5), sr, 32000).cpu()[0]
    assert float((dc[200:-200] - 0.5).abs().max()) < 1e-3      # a width-6 windowed sinc has ~5e-4 DC ripple
    t = np.arange(n) / sr
    # the width-6 window gives a wide transition band: 1 kHz passes to 2e-4, 12 kHz loses 1.5 %, the cut-off (0.99 x 16 kHz)
    # is the half-amplitude point, 20 kHz (aliasing to 12 kHz if it leaked) is down to 0.7 %
    for f, lo, hi, tol in ((1000.0, None, None, 1e-3), (12000.0, None, None, 3e-2), (15900.0, 0.35, 0.65, None),
                           (20000.0, 0.0, 1e-2, None)):
        x = torch.from_numpy(np.sin(2 * np.pi * f * t).astype(np.float32))[None]
        y = engine_f32.resample(x, sr, 32000).cpu()[0].numpy()
        mid = y[500:-500]
        if tol is not None:
            ref = np.sin(2 * np.pi * f * np.arange(len(y)) / 32000.0)[500:-500]
            assert np.abs(mid - ref).max() < tol, f
        else:
            assert lo <= np.abs(mid).max() < hi, f


def test_wrapper_device_resample_path_equals_host_path(synth_sd, tmp_path, monkeypatch):
    """MELLOW_DEVICE_RESAMPLE=1: wav -> GPU resampler -> tile/cat on torch's stream -> engine (own stream).  The engine must
    see completed tensors (stream hand-over); the texts equal the host-resampler path's."""
    from mellow_amd import MellowWrapper
    rng = np.random.default_rng(11)
    t1 = np.arange(int(2.7 * 44100)) / 44100.0
    p1, p2 = tmp_path / "a.wav", tmp_path / "b.wav"
    _write_wav16(p1, 0.3 * np.sin(2 * np.pi * 523 * t1) + 0.05 * rng.standard_normal(t1.size), 44100)
    t2 = np.arange(int(4.1 * 48000)) / 48000.0
    _write_wav16(p2, 0.2 * np.sin(2 * np.pi * 2100 * t2) + 0.05 * rng.standard_normal(t2.size), 48000)
    m = MellowWrapper(config="v0", model="v0", device=0, use_cuda=True, state_dict=synth_sd, tokenizer=_StubTokenizer())
    examples = [[str(p1), str(p2), "what differs"], [str(p2), str(p1), "which one is louder"], [str(p1), str(p1), "same"]]
    host = m.generate(examples=examples, max_len=8, top_p=0.8, temperature=1.0)
    monkeypatch.setenv("MELLOW_DEVICE_RESAMPLE", "1")
    for _ in range(3):          # repeated: a missing hand-over shows up as run-to-run differences
        dev = m.generate(examples=examples, max_len=8, top_p=0.8, temperature=1.0)
        assert dev == host
    m.model.close()
