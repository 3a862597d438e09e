"""f16 range safety.  Every other parity test runs on the N(0, 1 / fan-in) filler, whose activations stay O(10); trained ViT-L / DINOv2
checkpoints carry a handful of residual-stream channels 10^2 - 10^3 x larger.  The "outlier" weight set (panst3r_amd.synthetic.OUTLIER_CHANNELS: the rows of
every residual-writing projection of the three backbones that feed four fixed channels, x S) reproduces that; full-size v2 against the fp32 CPU oracle with the
SAME weights, tolerances = SURVEY 8(d) (bench.TOLERANCE), unrelaxed:
  S = 1e3   every placement - fp16, bf16 (f16 panoptic decoder), bf16 everywhere - stays finite and inside the five tolerances; the telemetry
            (hip.maxabs_telemetry) shows the largest 16-bit value, the 16-bit copy of the decoder's residual stream, at ~0.2 of the f16 range
  S = 3e4   the f16 backbone overflows; the call falls back by itself (PanSt3R.range_fallback_of: fp16 -> bf16 backbone + f16 panoptic decoder), says so in a
            RuntimeWarning, records the placement that ran in `last_precision`, and its outputs are inside the tolerances; range_fallback=False raises.
            An explicit panoptic placement ('reference': fp32 panoptic decoder) survives the fallback: only the backbone format moves.
Measured (profiles/r6_range_probe.txt): S = 1e3 fp16 pointmaps 5.4e-4 / masks 2.4e-3 / 99.96 %; bf16 5.0e-3 / 6.7e-3 / 99.87 %; S = 3e4 after the fallback 3.4e-3 / 8.6e-3 / 99.80 %."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def build_outlier(S):
    from panst3r_amd import hip
    from panst3r_amd.panst3r import CONFIG_V2, build_from_config
    from panst3r_amd.synthetic import fill_module_, synth_class_embeddings
    hip.lib()
    model = build_from_config(CONFIG_V2).eval()
    fill_module_(model, seed=1, outlier=S)
    names, emb = synth_class_embeddings(100)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.panoptic_decoder.text_encoder.class_embeddings = {n: e for n, e in zip(names, emb)}
    model.to(torch.device(DEV))
    return model, state, names, emb


def oracle(built, V, K):
    import bench
    model, state, names, emb = built
    _, ref, imgs, ts = bench.cpu_baseline('v2', 384, 512, state, names, emb, bench.usable_cores(), V=V, K=K)
    return ref, imgs, ts


def test_outlier_set_really_has_outlier_channels():
    """the set does what it says: the 16-bit copy of the residual streams reaches 10^3 - 10^4 (the plain filler: O(10)), far from uniform over the channels"""
    from panst3r_amd import hip
    from panst3r_amd.synthetic import synth_image
    built = build_outlier(1e3)
    model, _, names, _ = built
    dev = torch.device(DEV)
    imgs = [synth_image(i, 384, 512).to(dev) for i in range(2)]
    with hip.maxabs_telemetry() as log:
        model.forward_inference_multi_ar(imgs, torch.tensor([[384, 512]] * 2), names, num_keyframes=2, amp='fp16', max_bs=1)
    rows = hip.maxabs_report(log)
    assert rows and all(r[2] < hip.F16_MAX for r in rows), rows[:4]
    streams = [r for r in rows if 'residual stream' in r[1]]
    assert streams and streams[0][2] > 1e3, streams[:4]                     # outlier channels in the streams ...
    assert {r[0] for r in rows} >= {'memory build', 'render (MUSt3R decoder vs. memory)', 'query decoder', 'InputMixer + upscaler'}     # ... and every stage reports


@pytest.mark.parametrize('amp,pp', [('fp16', None), ('bf16', None), ('bf16', 'amp')])
def test_outlier_set_every_placement_within_the_stated_tolerances(amp, pp):
    import bench
    built = build_outlier(1e3)
    model, _, names, _ = built
    ref, imgs, ts = oracle(built, 2, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                    # no fallback may be needed at S = 1e3
        par = bench.full_size_parity(model, torch.device(DEV), ref, imgs, ts, names, amp=amp, K=2, panoptic_precision=pp)
    assert model.last_precision == (amp, pp)
    assert par['within_tolerance'], par
    assert par['decisions_matched']['within_tolerance_every_view'] or amp == 'bf16', par      # (bf16 on a 2-view scene: sign agreement 99.3-99.5 % per view, FULL_BOUNDS['bf16_2views'])


def test_f16_overflow_falls_back_to_a_range_safe_placement_by_itself():
    import bench
    built = build_outlier(3e4)
    model, _, names, _ = built
    ref, imgs, ts = oracle(built, 2, 2)
    dev = torch.device(DEV)
    inp = [i.to(dev) for i in imgs]
    with pytest.raises(FloatingPointError):
        model.forward_inference_multi_ar(inp, ts, names, num_keyframes=2, amp='fp16', max_bs=1, range_fallback=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        pm, pan = model.forward_inference_multi_ar(inp, ts, names, num_keyframes=2, amp='fp16', max_bs=1)
    assert any('repeating the call' in str(x.message) for x in w), [str(x.message) for x in w]
    assert model.last_precision == ('bf16', None)
    assert all(bool(torch.isfinite(t).all()) for t in pm) and all(bool(torch.isfinite(t).all()) for t in pan['pred_masks'])
    e = bench._scene_errors(pm, pan, ref[0], ref[1])
    assert bench._within(e), e


def test_f16_overflow_fallback_keeps_an_explicit_panoptic_placement():
    """amp='fp16', panoptic_precision='reference' at S = 3e4: the fallback moves the backbone to bf16 and keeps the caller's fp32 panoptic placement
    (it used to drop it and put the panoptic decoder on f16 operands)."""
    import bench
    from panst3r_amd.panst3r import PanSt3R
    assert PanSt3R.range_fallback_of('fp16', 'reference') == ('bf16', 'reference')
    built = build_outlier(3e4)
    model, _, names, _ = built
    ref, imgs, ts = oracle(built, 2, 2)
    inp = [i.to(torch.device(DEV)) for i in imgs]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        pm, pan = model.forward_inference_multi_ar(inp, ts, names, num_keyframes=2, amp='fp16', max_bs=1, panoptic_precision='reference')
    assert any('repeating the call' in str(x.message) for x in w), [str(x.message) for x in w]
    assert model.last_precision == ('bf16', 'reference')
    assert all(bool(torch.isfinite(t).all()) for t in pm) and all(bool(torch.isfinite(t).all()) for t in pan['pred_masks'])
    e = bench._scene_errors(pm, pan, ref[0], ref[1])
    assert bench._within(e), e
