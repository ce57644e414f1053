"""GPU: the reduced-precision arm (bf16 MFMA for the transformer's dense layers and the decoder's convolutions).
Kernel-level: exact agreement with an fp64 reference evaluated on bf16-rounded operands (products of bf16 values
are exact in fp32, so only the summation order differs) — this pins the fragment layouts.  Model-level: the
STATED tolerances of the arm against the fp32/fp64 oracle, and bit-exact context tokens (the encoder stays fp32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# ---- stated tolerances of the bf16 arm (north star: "logits and decoded pixels within a stated fp tolerance") ----
LOGIT_TOL_REL = 3e-2        # max |logit error| / max |logit|, 12-layer MIGT with bf16 dense layers
PIXEL_TOL_ABS = 8e-2        # max |decoded pixel error| on the [-1, 1] scale, bf16 decoder (measured 5.7e-2 .. 6.1e-2: the
                            # maximum over 98k pixels moves with any last-bit change upstream; the mean is 4.4e-3)
PIXEL_TOL_MEAN = 6e-3       # mean |decoded pixel error|
U8_TOL_LEVELS = 10          # max uint8 level difference of the final image (measured 7 .. 8)
# VQGAN.decoder_act16 = 64 / 32 (bf16 activations between the decoder's layers from 64^2 / 32^2 up; the default, 128, stays inside the bounds above:
# measured 6.4e-2 / 4.6e-3 / 8 levels)
ACT16_PIXEL_TOL_ABS = 1.1e-1     # measured 6.9e-2 (64), 8.1e-2 (32)
ACT16_PIXEL_TOL_MEAN = 7e-3      # measured 4.9e-3, 5.3e-3
ACT16_U8_TOL_LEVELS = 13         # measured 9, 10


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _rand(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _bf(x):
    return x.to(torch.bfloat16).double()


def _rel(a, b):
    b = torch.as_tensor(b).double()
    return ((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize('M,K,N', [(128, 64, 128), (300, 128, 64), (448, 768, 2304), (1000, 3072, 768), (70, 256, 1024),
                                   (1024, 64, 128), (1500, 768, 200), (2048 + 37, 192, 768)])      # M >= 1024: the 256-row-tile kernel
def test_gemm_bf16_layout_and_epilogue(dev, M, K, N):
    from viewformer_amd import ops
    x, w, b, r = _rand((M, K), 1), _rand((K, N), 2, 0.1), _rand((N,), 3), _rand((M, N), 4)
    for epi in (ops.EPI_NONE, ops.EPI_GELU):
        out = torch.empty((M, N), device=dev)
        ops.igemm(x.to(dev), ops.pack_dense_kn_bf16(w.to(dev)), M, K, N, out, bias=b.to(dev), res=r.to(dev), epilogue=epi, bf16=True)
        ref = _bf(x) @ _bf(w) + b.double()
        if epi == ops.EPI_GELU:
            ref = F.gelu(ref)
        ref = ref + r.double()
        assert _rel(out, ref) < 2e-5, (M, K, N, epi)
    out2 = torch.empty((M, N), device=dev)
    ops.igemm(x.to(dev), ops.pack_dense_nk_bf16(w.t().contiguous().to(dev)), M, K, N, out2, bf16=True)
    assert _rel(out2, _bf(x) @ _bf(w)) < 2e-5
    with pytest.raises(ops._lib.VfError):          # K % 64 != 0 is refused, never silently rerouted
        ops.igemm(x[:, :32].contiguous().to(dev), ops.pack_dense_kn_bf16(w[:32].contiguous().to(dev)), M, 32, N, out2, bf16=True)


@pytest.mark.parametrize('mode,cin,cout,H,pro', [('s1', 128, 128, 16, True), ('s1', 64, 256, 32, False), ('up', 128, 128, 8, False),
                                                  ('up', 32, 128, 16, True), ('s1', 256, 128, 64, True),
                                                  ('s1', 128, 128, 8, True), ('s1', 512, 512, 8, False)])
def test_conv3_halo_bf16(dev, mode, cin, cout, H, pro):
    from viewformer_amd import ops
    n = 3 if H == 8 else 2
    x = _rand((n, cin, H, H), 11) * 1.5 + 0.2
    w, b = _rand((cout, cin, 3, 3), 12, 0.05), _rand((cout,), 13)
    gamma, beta = _rand((cin,), 14) * 0.3 + 1, _rand((cin,), 15) * 0.2
    xd = x.double()
    a = xd
    if pro:
        a = F.group_norm(xd, 32, gamma.double(), beta.double(), eps=1e-6)
        a = a * torch.sigmoid(a)
    a = _bf(a.float())                                         # operand rounding of the arm
    wq = _bf(w)
    if mode == 's1':
        ref, m, Ho = F.conv2d(a, wq, b.double(), padding=1), ops.MODE_CONV3_S1, H
    else:
        ref, m, Ho = F.conv2d(F.interpolate(a, scale_factor=2.0, mode='nearest'), wq, b.double(), padding=1), ops.MODE_CONV3_UP2, H * 2
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    prol = None
    if pro:
        mean_c, scale_c = ops.groupnorm_stats(xn, gamma.to(dev), n, H * H, cin)
        prol = (mean_c, scale_c, beta.to(dev))
    res = _rand((n * Ho * Ho, cout), 16)
    out = torch.empty((n * Ho * Ho, cout), device=dev)
    ops.igemm(xn, ops.pack_conv3_bf16(w.to(dev)), n * Ho * Ho, cin, cout, out, bias=b.to(dev), res=res.to(dev), mode=m, pro=prol,
              pro_swish=True, Hin=H, Win=H, Hout=Ho, Wout=Ho, bf16=True)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, cout) + res.double()
    # with the prologue the activation is rounded to bf16 AFTER an fp32 transform whose last bits differ from the fp64
    # reference's, so a few operands land on the neighbouring bf16 value: allow one-ulp-of-bf16-sized noise there
    assert _rel(out, ref) < (3e-3 if pro else 3e-5), (mode, cin, cout, pro, _rel(out, ref))


@pytest.mark.parametrize('mode,cin,cout,H,pro,a16,with_res', [('s1', 128, 128, 16, True, True, True), ('s1', 256, 128, 32, True, True, False),
                                                               ('up', 256, 256, 16, False, False, False), ('up', 128, 128, 16, False, True, False),
                                                               ('s1', 64, 256, 32, False, True, True), ('s1', 128, 128, 64, True, True, True)])
def test_conv3_halo_bf16_with_bf16_activations_rounds_the_fp32_result(dev, mode, cin, cout, H, pro, a16, with_res):
    """vf_conv3_halo_bf16 with reserved0 bit 1 (bf16 out + residual) and bit 0 (bf16 in): the SAME accumulators as the fp32-activation
    launch on the widened operands, rounded once at the store; the fused GroupNorm partials are those of the fp32 values"""
    from viewformer_amd import ops
    n = 2
    x16 = (_rand((n * H * H, cin), 21) * 1.5 + 0.2).to(torch.bfloat16).to(dev)
    x32 = x16.float()
    w, b = _rand((cout, cin, 3, 3), 22, 0.05), _rand((cout,), 23)
    gamma, beta = _rand((cin,), 24) * 0.3 + 1, _rand((cin,), 25) * 0.2
    m, Ho = (ops.MODE_CONV3_S1, H) if mode == 's1' else (ops.MODE_CONV3_UP2, 2 * H)
    prol = None
    if pro:
        mean_c, scale_c = ops.groupnorm_stats(x32, gamma.to(dev), n, H * H, cin)
        prol = (mean_c, scale_c, beta.to(dev))
    M = n * Ho * Ho
    res16 = _rand((M, cout), 26).to(torch.bfloat16).to(dev) if with_res else None
    wp = ops.pack_conv3_bf16(w.to(dev))
    kw = dict(bias=b.to(dev), mode=m, pro=prol, pro_swish=True, Hin=H, Win=H, Hout=Ho, Wout=Ho, bf16=True)
    out32, part32 = torch.empty((M, cout), device=dev), ops.new_gn_part(n, Ho, Ho, dev)
    ops.igemm(x32, wp, M, cin, cout, out32, res=res16.float() if with_res else None, gn_part=part32, **kw)
    out16, part16 = torch.empty((M, cout), dtype=torch.bfloat16, device=dev), ops.new_gn_part(n, Ho, Ho, dev)
    ops.igemm(x16 if a16 else x32, wp, M, cin, cout, out16, res=res16, gn_part=part16, a16=a16, o16=True, **kw)
    assert torch.equal(out16, out32.to(torch.bfloat16))
    g32 = ops.groupnorm_finalize(part32, gamma[:1].expand(cout).contiguous().to(dev), n, Ho * Ho, cout, 32, 1e-6)
    g16 = ops.groupnorm_finalize(part16, gamma[:1].expand(cout).contiguous().to(dev), n, Ho * Ho, cout, 32, 1e-6)
    assert torch.equal(g16[0], g32[0]) and torch.equal(g16[1], g32[1])
    with pytest.raises(ops._lib.VfError):             # bf16 in with fp32 out is not an arm of the kernel
        ops.igemm(x16, wp, M, cin, cout, out32, a16=True, **kw)
    if with_res:
        with pytest.raises(TypeError):                # bf16 out takes its residual as bf16 too
            ops.igemm(x16, wp, M, cin, cout, out16, res=res16.float(), a16=True, o16=True, **kw)


def test_conv3_small_cout_reads_bf16_activations(dev):
    from viewformer_amd import ops
    n, H, C = 2, 64, 128
    x16 = (_rand((n * H * H, C), 31) * 1.2).to(torch.bfloat16).to(dev)
    w, b = _rand((3, C, 3, 3), 32, 0.05).to(dev), _rand((3,), 33).to(dev)
    gamma, beta = (_rand((C,), 34) * 0.3 + 1).to(dev), (_rand((C,), 35) * 0.2).to(dev)
    mean_c, scale_c = ops.groupnorm_stats(x16.float(), gamma, n, H * H, C)
    for pro in (None, (mean_c, scale_c, beta)):
        a = ops.conv3_small_cout(x16, w, b, n, H, H, C, 3, pro=pro)
        r = ops.conv3_small_cout(x16.float(), w, b, n, H, H, C, 3, pro=pro)
        assert torch.equal(a, r)


def test_migt_bf16_logits_within_stated_tolerance(dev):
    from oracle import migt_oracle as mg
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    cfg = MIGTConfig(sequence_size=7, localization_weight='1', pose_multiplier=0.2)
    sd = make_migt_weights(cfg, seed=0)
    g = np.random.Generator(np.random.PCG64(17))
    B, S = 2, 7
    codes = torch.from_numpy(g.integers(0, 1024, size=(B, S, 8, 8)))
    _, cams = synthetic_scene_batch(B, S, 8, 6)
    cams = mg.normalize_cameras(mg.to_relative_cameras(torch.from_numpy(cams))[0])
    m16 = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    m32 = MIGT(cfg, precision='f32').load_state_dict(sd).to(dev)
    lg16, pose16 = m16.generate_and_localize(codes.to(dev), cams.to(dev))
    lg32, pose32 = m32.generate_and_localize(codes.to(dev), cams.to(dev))
    ids = torch.cat([codes[:, :-1], torch.full_like(codes[:, :1], 1024)], 1)
    ref = mg.migt_forward(sd, cfg, ids, cams, dtype=torch.float64)['logits'][:, -1]
    e16, e32 = _rel(lg16, ref), _rel(lg32, ref)
    agree = (lg16.argmax(-1).cpu() == ref.argmax(-1)).float().mean().item()
    print(f'logit rel err: bf16 arm {e16:.2e}, fp32 arm {e32:.2e}; arg-max agreement of the bf16 arm {agree:.3f} '
          f'(random-init logits are nearly flat: |logit| max {ref.abs().max():.2f})')
    assert e32 < 1e-4 and e16 < LOGIT_TOL_REL
    assert _rel(pose16, pose32.cpu()) < 5e-2


def test_decoder_bf16_pixels_within_stated_tolerance_and_tokens_stay_exact(dev, full_vq):
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import synthetic_scene_batch
    cfg, sd, g = full_vq
    m16 = VQGAN(cfg, data_format='NHWC', decoder_precision='bf16').load_state_dict(sd).to(dev)
    frames, _ = synthetic_scene_batch(1, 4, 128, seed=int(g['input_seed']))
    codes = m16.encode(torch.from_numpy(frames[0]).to(dev))[-1]
    assert np.array_equal(codes.cpu().numpy(), g['codes'])             # the encoder is untouched: bit-exact tokens
    dec = m16.decode_code(torch.from_numpy(g['codes'][:2]).to(dev)).permute(0, 3, 1, 2).cpu()
    err = (dec.double() - torch.from_numpy(g['decoded']).double()).abs()
    from oracle import vqgan_oracle as vq
    u16, u32 = vq.postprocess_u8(dec), vq.postprocess_u8(torch.from_numpy(g['decoded']))
    du = (u16.int() - u32.int()).abs()
    print(f'bf16 decoder: max |pixel err| {err.max():.3e} (mean {err.mean():.2e}); uint8 max diff {du.max().item()}, '
          f'{(du > 1).float().mean().item():.4f} of pixels differ by > 1 level')
    assert err.max() < PIXEL_TOL_ABS and err.mean() < PIXEL_TOL_MEAN and du.max() <= U8_TOL_LEVELS
    # bf16 activations between the decoder's layers from R x R up (decoder_act16 = R; default 128, inside the tolerance above): fp32
    # activations throughout (0) inside it too; the wider forms carry their own, looser, stated tolerance
    assert m16.decoder_act16 == 128
    for R in (0, 64, 32):
        m16.decoder_act16 = R
        dec2 = m16.decode_code(torch.from_numpy(g['codes'][:2]).to(dev)).permute(0, 3, 1, 2).cpu()
        err2 = (dec2.double() - torch.from_numpy(g['decoded']).double()).abs()
        du2 = (vq.postprocess_u8(dec2).int() - u32.int()).abs()
        print(f'  decoder_act16={R}: max |pixel err| {err2.max():.3e} (mean {err2.mean():.2e}); uint8 max diff {du2.max().item()}')
        wide = R != 0
        assert err2.max() < (ACT16_PIXEL_TOL_ABS if wide else PIXEL_TOL_ABS) and err2.mean() < (ACT16_PIXEL_TOL_MEAN if wide else PIXEL_TOL_MEAN)
        assert du2.max() <= (ACT16_U8_TOL_LEVELS if wide else U8_TOL_LEVELS)
        assert not torch.equal(dec, dec2)                               # (the switch does something)
    m16.decoder_act16 = 128


@pytest.mark.parametrize('ch', [64])       # (ch = 96: the standalone GroupNorm kernel takes power-of-two channel counts only — that config never ran)
def test_decoder_bf16_arm_with_a_top_level_the_bf16_activation_stream_cannot_take(dev, ch):
    """decoder_act16 (default 128) switched the activation stream to bf16 at the last upsample convolution without
    asking whether the layers behind it can read bf16 — with ch = 64 (top level 64 channels: no bf16 halo packing, no fused GroupNorm
    statistics) the decode raised, where round 3's per-layer fp32 fallback ran.  The switch is now decided from the decoder plan
    (every conv / norm / shortcut up to conv_out must qualify): such configs keep fp32 activations and decode within the bf16 arm's bound."""
    from oracle import vqgan_oracle as vq
    from viewformer_amd.config import VQGANConfig
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_vqgan_weights
    cfg = VQGANConfig(ch=ch, ch_mult=[1, 2, 4], num_res_blocks=1, attn_resolutions=[], image_size=128, z_channels=64, embed_dim=64, n_embed=128)
    sd = make_vqgan_weights(cfg, seed=3, codebook_scale=0.05)
    codes = torch.from_numpy(np.random.default_rng(5).integers(0, 128, size=(2, 32, 32)))
    ref = vq.decode_code(sd, cfg, codes, dtype=torch.float64)
    for R in (128, 64, 32, 0):
        m = VQGAN(cfg, data_format='NCHW', decoder_precision='bf16').load_state_dict(sd).to(dev)
        m.decoder_act16 = R
        dec = m.decode_code(codes.to(dev)).cpu()
        err = (dec.double() - ref).abs()
        print(f'ch={ch} decoder_act16={R}: max |pixel err| {err.max():.3e} (mean {err.mean():.2e}), |ref| max {ref.abs().max():.2f}')
        assert err.max() < ACT16_PIXEL_TOL_ABS * max(1.0, float(ref.abs().max())) and dec.dtype == torch.float32
    m32 = VQGAN(cfg, data_format='NCHW').load_state_dict(sd).to(dev)
    assert (m32.decode_code(codes.to(dev)).cpu().double() - ref).abs().max() < 2e-4 * max(1.0, float(ref.abs().max()))


def test_pipeline_bf16_arm(dev, full_vq):
    """end to end with both arms on: context tokens bit-exact vs the oracle, logits within the stated tolerance"""
    from oracle import pipeline_oracle as po
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.evaluate import generate_batch_predictions
    from viewformer_amd.migt import MIGT
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    mcfg = MIGTConfig(sequence_size=3, localization_weight='1', pose_multiplier=0.2, n_layer=4)
    msd = make_migt_weights(mcfg, seed=1)             # the reference's init scale (std 0.02), like the bench
    frames, cams = synthetic_scene_batch(2, 3, 128, seed=3)
    ref = po.generate_batch_predictions(msd, mcfg, vsd, vcfg, frames, cams, return_intermediates=True)
    vq_m = VQGAN(vcfg, data_format='NHWC', decoder_precision='bf16').load_state_dict(vsd).to(dev)
    tr_m = MIGT(mcfg, precision='bf16').load_state_dict(msd).to(dev)
    got = generate_batch_predictions(tr_m, vq_m, frames, cams, return_codes=True)
    assert torch.equal(got['codes'].cpu(), ref['codes'])
    assert _rel(got['logits_last'], ref['logits_last']) < LOGIT_TOL_REL
    assert got['generated_images'].dtype == torch.uint8


ATTN_TOL = 1.5e-2       # max |attention output error| / max |output|: bf16 Q, K, V and probabilities, fp32 softmax and sums
DMA_VS_LP_TOL = 1.0e-2  # between the two bf16 attention kernels (same operands; since round 4 different rounding points in the softmax)


@pytest.mark.parametrize('B,H,S,L,mode', [(2, 2, 4, 16, 'causal'), (1, 12, 7, 64, 'causal'), (1, 2, 5, 48, 'causal'),
                                          (2, 3, 8, 64, 'twin'), (1, 2, 3, 64, 'streams')])
def test_attention_bf16_all_mask_modes(dev, B, H, S, L, mode):
    """bf16-MFMA attention against the SAME kernel contract in exact fp32 (vf_attn_blockcausal_f32, itself pinned to the
    oracle's compute_causal_block[_multiend]_attention): plain block-causal, twin views, streams; skip == dense."""
    from viewformer_amd import ops
    d = H * 64
    NS = 3 if mode == 'streams' else 1
    T = NS * S * L
    spec = {'causal': -1, 'twin': S - 2, 'streams': -S}[mode]
    qkv = _rand((B * T, 3 * d), 71, 0.35).to(dev)
    ref = torch.empty((B * T, d), device=dev)
    ops.attn_blockcausal(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], ref, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 1.0, True, spec)
    outs = []
    for skip in (True, False):
        out = torch.empty((B * T, d), device=dev)
        ops.attn_blockcausal(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], out, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 1.0, skip, spec,
                             bf16=True)
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        assert err < ATTN_TOL, (mode, skip, err)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])        # skipping fully masked tiles == the dense "-1e4" form, also in bf16
    print(f'bf16 attention {mode} B={B} H={H} S={S} L={L}: rel err {err:.2e}')


@pytest.mark.parametrize('B,H,S,mode', [(1, 12, 7, 'causal'), (2, 3, 8, 'twin'), (1, 2, 3, 'streams'), (3, 2, 1, 'causal'), (2, 2, 5, 'twin'),
                                        (1, 2, 21, 'twin')])
def test_attention_dma_kernel_against_the_register_staged_kernel_and_the_exact_one(dev, B, H, S, mode):
    """bf16 q/k/v in, bf16 out, 64-token views: the LDS-DMA ring kernel (attention_dma.hip) against attention_lp.hip on the same
    inputs (vf_select(VF_SEL_ATTN_DMA, 0)) and against the exact fp32 kernel.  Until round 3 the two bf16 kernels were bit-identical; round 4
    folded the softmax's scale and maximum into the MFMA (q re-rounded to bf16 after the multiplication by scale * log2 e, score
    accumulators started at minus a reference maximum that moves only past a threshold): the same softmax evaluated with other
    rounding points, so the two now agree to DMA_VS_LP_TOL and each stays within ATTN_TOL of the exact kernel.  Covers one-view
    sequences, sequences that do not fill the last 4-view workgroup, and 21-view sequences (S = 20 + twin)."""
    from viewformer_amd import ops
    L, d = 64, H * 64
    NS = 3 if mode == 'streams' else 1
    T = NS * S * L
    spec = {'causal': -1, 'twin': max(S - 2, 0), 'streams': -S}[mode]
    qkv = _rand((B * T, 3 * d), 91, 0.35).to(dev)
    q16 = qkv.to(torch.bfloat16)
    ref = torch.empty((B * T, d), device=dev)
    ops.attn_blockcausal(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], ref, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 0.7, True, spec)
    outs = {}
    from viewformer_amd import _lib
    for flag in ('1', '0'):
        prev = _lib.select(_lib.SEL_ATTN_DMA, flag == '1')
        try:
            out = torch.full((B * T, d), float('nan'), dtype=torch.bfloat16, device=dev)
            ops.attn_blockcausal(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], out, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 0.7, True, spec, bf16=True)
        finally:
            _lib.select(_lib.SEL_ATTN_DMA, prev)
        outs[flag] = out
    assert not torch.isnan(outs['1'].float()).any()
    e_lp = ((outs['1'].float() - outs['0'].float()).abs().max() / ref.abs().max()).item()
    err = ((outs['1'].float() - ref).abs().max() / ref.abs().max()).item()
    err_lp = ((outs['0'].float() - ref).abs().max() / ref.abs().max()).item()
    print(f'attention {mode} B={B} H={H} S={S}: dma vs exact {err:.2e}, lp vs exact {err_lp:.2e}, dma vs lp {e_lp:.2e}')
    assert e_lp < DMA_VS_LP_TOL, e_lp
    assert err < ATTN_TOL and err_lp < ATTN_TOL, (err, err_lp)
    # ... and it is deterministic, and a query's result does not depend on the other scenes / heads in the launch
    out2 = torch.full((B * T, d), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.attn_blockcausal(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], out2, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 0.7, True, spec, bf16=True)
    assert torch.equal(out2, outs['1'])
    if B > 1:
        one = torch.full((T, d), float('nan'), dtype=torch.bfloat16, device=dev)
        q1 = q16[T:2 * T].contiguous()
        ops.attn_blockcausal(q1[:, d:2 * d], q1[:, 2 * d:], q1[:, :d], one, 1, H, T, L, 3 * d, 3 * d, 3 * d, d, 0.7, True, spec, bf16=True)
        assert torch.equal(one, outs['1'][T:2 * T])


@pytest.mark.parametrize('B,H,S,mode', [(3, 4, 8, 'twin'), (2, 2, 10, 'streams'), (1, 3, 7, 'causal'), (2, 1, 1, 'causal'), (1, 2, 21, 'twin'), (2, 2, 3, 'streams'),
                                        (1, 12, 5, 'twin')])
def test_attention_dma_32_query_waves_are_bit_identical_to_64_query_waves(dev, B, H, S, mode):
    """the two wave shapes of the LDS-DMA kernel — 8 waves x 32 queries (round 4, the default) and 4 waves x 64 queries — run the same
    per-query operations in the same order: identical bits in every mask mode, for blocks whose last views do not exist, one-view and
    21-view sequences; with and without the log-sum-exp output and attention dropout (the training forward)"""
    from viewformer_amd import ops, _lib
    from viewformer_amd import train_ops as T
    L, d = 64, H * 64
    NS = 3 if mode == 'streams' else 1
    Tn = NS * S * L
    spec = {'causal': -1, 'twin': max(S - 2, 0), 'streams': -S}[mode]
    q16 = _rand((B * Tn, 3 * d), 99, 0.35).to(dev).to(torch.bfloat16)
    res = {}
    for flag in (1, 0):
        prev = _lib.select(_lib.SEL_ATTN_Q32, flag)
        try:
            out = torch.full((B * Tn, d), float('nan'), dtype=torch.bfloat16, device=dev)
            ops.attn_blockcausal(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], out, B, H, Tn, L, 3 * d, 3 * d, 3 * d, d, 0.7, True, spec, bf16=True)
            o2 = torch.full((B * Tn, d), float('nan'), dtype=torch.bfloat16, device=dev)
            lse = T.attn_fwd_lse_bf16(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], o2, B, H, Tn, L, 3 * d, 3 * d, 3 * d, d, 0.7, spec)
            o3 = torch.full((B * Tn, d), float('nan'), dtype=torch.bfloat16, device=dev)
            lse3 = T.attn_fwd_lse_bf16(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], o3, B, H, Tn, L, 3 * d, 3 * d, 3 * d, d, 0.7, spec, drop=(0.1, 5, 20, 24))
        finally:
            _lib.select(_lib.SEL_ATTN_Q32, prev)
        res[flag] = (out, o2, lse, o3, lse3)
    assert not torch.isnan(res[1][0].float()).any() and not torch.isnan(res[1][3].float()).any()
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)
    assert torch.equal(res[1][0], res[1][1]) and torch.equal(res[1][2], res[1][4])      # (the lse output changes nothing; dropout does not touch it)


# (The bit-identity tests of round 3's three slower forms of this kernel — 8-wave, resident, software-pipelined — left with the kernels,
# whose sources were last kept in tools/variants/attention_dma_r3_records.hip at commit 9158f1d; they passed on MI355X at commit 7e8c4c4,
# GPUTEST_r03.json.)


def test_bf16_activation_chain_is_bit_identical(dev):
    """LayerNorm / GELU / attention outputs written as bf16 by their producers and read as bf16 by the GEMMs (a16 / o16): the same
    rounding the GEMM applies to an fp32 operand on load, so everything downstream is bit-identical — kernel by kernel and for the
    full-size transformer's logits"""
    from viewformer_amd import ops
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    from oracle import migt_oracle as mg
    M, K, N = 300, 256, 384
    x, w, b = _rand((M, K), 61).to(dev), _rand((K, N), 62, 0.1).to(dev), _rand((N,), 63).to(dev)
    wp = ops.pack_dense_kn_bf16(w)
    g, be = (_rand((K,), 64) * 0.3 + 1).to(dev), _rand((K,), 65).to(dev)
    ln32, ln16 = ops.layernorm(x, g, be, M, K), ops.layernorm(x, g, be, M, K, out_bf16=True)
    assert ln16.dtype == torch.bfloat16 and torch.equal(ln16, ln32.to(torch.bfloat16))
    for epi in (ops.EPI_NONE, ops.EPI_GELU):
        o_ref, o_a16 = torch.empty((M, N), device=dev), torch.empty((M, N), device=dev)
        ops.igemm(ln32, wp, M, K, N, o_ref, bias=b, epilogue=epi, bf16=True)
        ops.igemm(ln16, wp, M, K, N, o_a16, bias=b, epilogue=epi, bf16=True, a16=True)
        assert torch.equal(o_ref, o_a16)
        o16 = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        ops.igemm(ln16, wp, M, K, N, o16, bias=b, epilogue=epi, bf16=True, a16=True, o16=True)
        assert torch.equal(o16, o_ref.to(torch.bfloat16))
    B, H, S, L, d = 2, 2, 3, 64, 128
    qkv = _rand((B * S * L, 3 * d), 66).to(dev)
    a32 = torch.empty((B * S * L, d), device=dev)
    a16 = torch.empty((B * S * L, d), dtype=torch.bfloat16, device=dev)
    for out in (a32, a16):
        ops.attn_blockcausal(qkv[:, d:2 * d], qkv[:, 2 * d:], qkv[:, :d], out, B, H, S * L, L, 3 * d, 3 * d, 3 * d, d, 0.3, True, -1, bf16=True)
    assert torch.equal(a16, a32.to(torch.bfloat16))
    q16 = qkv.to(torch.bfloat16)                              # bf16 q/k/v (the c_attn GEMM's o16 output) == fp32 q/k/v of the same values
    a_in16, a_ref = torch.empty_like(a32), torch.empty_like(a32)
    ops.attn_blockcausal(q16[:, d:2 * d], q16[:, 2 * d:], q16[:, :d], a_in16, B, H, S * L, L, 3 * d, 3 * d, 3 * d, d, 0.3, True, -1, bf16=True)
    qr = q16.float()
    ops.attn_blockcausal(qr[:, d:2 * d], qr[:, 2 * d:], qr[:, :d], a_ref, B, H, S * L, L, 3 * d, 3 * d, 3 * d, d, 0.3, True, -1, bf16=True)
    assert torch.equal(a_in16, a_ref)
    # whole transformer
    cfg = MIGTConfig(sequence_size=4, localization_weight='1', pose_multiplier=0.2)
    sd = make_migt_weights(cfg, seed=0)
    gen = np.random.Generator(np.random.PCG64(17))
    codes = torch.from_numpy(gen.integers(0, 1024, size=(2, 4, 8, 8)))
    _, cams = synthetic_scene_batch(2, 4, 8, 6)
    cams = mg.normalize_cameras(mg.to_relative_cameras(torch.from_numpy(cams))[0])
    from viewformer_amd import _lib
    outs = []
    prev = _lib.select(_lib.SEL_ATTN_DMA, 0)                   # (both forms on the register-staged attention: the LDS-DMA kernel, which only the
    try:                                                      # bf16-activation form can take, has had its own rounding points since round 4)
        for flag in (False, True):
            m = MIGT(cfg, precision='bf16', bf16_activations=flag).load_state_dict(sd).to(dev)
            lg, pose = m.generate_and_localize(codes.to(dev), cams.to(dev))
            outs.append((lg, pose))
    finally:
        _lib.select(_lib.SEL_ATTN_DMA, prev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    lg_dma, pose_dma = m.generate_and_localize(codes.to(dev), cams.to(dev))             # the product path (LDS-DMA attention)
    e = ((lg_dma - outs[1][0]).abs().max() / outs[1][0].abs().max()).item()
    print('12-layer logits, LDS-DMA attention vs register-staged attention:', e)
    assert e < 1e-2, e


@pytest.mark.parametrize('M,K,N', [(512, 128, 256), (1000, 768, 768), (2048, 768, 2304), (1290, 3072, 768), (4096, 768, 3072), (770, 256, 1280),
                                   (1536, 256, 512), (2048, 128, 2048)])
def test_gemm_bf16_256_tile_lds_dma_kernel_is_bit_identical(dev, M, K, N):
    """the 256 x 256 LDS-DMA kernel (gemm_bf16_g256.hip, taken for bf16 activations and 256-aligned widths) against the 128 x 128 kernel
    (vf_select(VF_SEL_GEMM_G256, 0)): same MFMA, same k order, fp32 epilogue -> the same bits; ragged last row tile, residual, GELU, bf16 output;
    and against the fp64 reference on the bf16-rounded operands"""
    from viewformer_amd import ops
    x = _rand((M, K), 71).to(dev).to(torch.bfloat16)
    w, b, r = _rand((K, N), 72, 0.05).to(dev), _rand((N,), 73).to(dev), _rand((M, N), 74).to(dev)
    wp = ops.pack_dense_kn_bf16(w)
    ref64 = x.double().cpu() @ _bf(w.cpu()) + b.double().cpu()

    def run(epi, res, o16):
        out = torch.full((M, N), float('nan'), dtype=torch.bfloat16 if o16 else torch.float32, device=dev)
        ops.igemm(x, wp, M, K, N, out, bias=b, epilogue=epi, res=res, bf16=True, a16=True, o16=o16)
        return out
    for epi, res, o16 in ((ops.EPI_NONE, None, False), (ops.EPI_NONE, r, False), (ops.EPI_GELU, None, True), (ops.EPI_NONE, None, True),
                          (ops.EPI_GELU, r, False)):
        from viewformer_amd import _lib
        new = run(epi, res, o16)
        prev = _lib.select(_lib.SEL_GEMM_G256, 0)
        try:
            old = run(epi, res, o16)
        finally:
            _lib.select(_lib.SEL_GEMM_G256, prev)
        assert not torch.isnan(new.float()).any()
        assert torch.equal(new, old), (epi, res is not None, o16, (new.float() - old.float()).abs().max().item())
    plain = run(ops.EPI_NONE, None, False)
    assert _rel(plain, ref64) < 2e-6


@pytest.mark.parametrize('M,K,N,tail', [(19200, 768, 3072, (64, 15, 3)), (19200, 768, 2304, (56, 26, 3)), (57344, 3072, 768, (170, 72, 3)),
                                        (19200 - 70, 128, 3072, (64, 15, 3)), (16384 + 4000, 128, 2048, (64, 32, 2)), (19200, 768, 768, None),
                                        (65536, 128, 3072, None)])
def test_gemm_bf16_tail_tiles_are_bit_identical_to_the_plain_grid(dev, M, K, N, tail):
    """round 6: launches whose last round of the 256 CUs would be partly filled end with one round of 192- / 128-row TAIL tiles instead
    (csrc/gemm_bf16_g256.hip: g256_tail_policy; vf_select(VF_SEL_GEMM_TAIL)).  K is never split, so every output element keeps its k order:
    the two grids must agree bit for bit — every epilogue form of the kernel, ragged ends inside a tail tile, no row written twice or left out
    (NaN-filled outputs), and the training / inference shapes the policy exists for really take it (`tail` = the expected (full row tiles,
    tail row tiles, 32-row blocks per wave group) per column; None = the plain grid)."""
    from viewformer_amd import _lib, ops
    mt, nb = -(-M // 256), N // 256
    ntiles = mt * nb
    # the policy, restated (csrc/gemm_bf16_g256.hip): the test pins which shapes take it
    exp = None
    last = ntiles % 256
    if ntiles > 256 and 16 <= last <= 184:
        f = (ntiles // 256) * 256 // nb
        rem = -(-(M - f * 256) // 32)
        for ic in (2, 3):
            h = -(-rem // (2 * ic))
            if h * nb <= 256:
                exp = (f, h, ic)
                break
    assert exp == tail, (exp, tail)
    x = _rand((M, K), 171).to(dev).to(torch.bfloat16)
    w, b = _rand((K, N), 172, 0.05).to(dev), _rand((N,), 173).to(dev)
    r, u16 = _rand((M, N), 174).to(dev), _rand((M, N), 175).to(dev).to(torch.bfloat16)
    wp = ops.pack_dense_kn_bf16(w)

    def run(form):
        o16 = form in ('bf16', 'gelu16', 'dual16', 'gbwd')
        out = torch.full((M, N), float('nan'), dtype=torch.bfloat16 if o16 else torch.float32, device=dev)
        aux = torch.full((M, N), float('nan'), dtype=torch.bfloat16, device=dev) if form in ('dual16', 'dual32') else None
        if form == 'f32res':
            ops.igemm(x, wp, M, K, N, out, bias=b, res=r, bf16=True, a16=True)
        elif form == 'drop':
            ops.igemm(x, wp, M, K, N, out, bias=b, res=r, bf16=True, a16=True, drop=(0.1, 11, 2, 8))
        elif form == 'bf16':
            ops.igemm(x, wp, M, K, N, out, bias=b, bf16=True, a16=True, o16=True)
        elif form == 'gelu16':
            ops.igemm(x, wp, M, K, N, out, bias=b, epilogue=ops.EPI_GELU, bf16=True, a16=True, o16=True)
        elif form in ('dual16', 'dual32'):
            ops.igemm(x, wp, M, K, N, out, bias=b, epilogue=ops.EPI_GELU_DUAL, bf16=True, a16=True, o16=o16, out_aux=aux)
        elif form == 'gbwd':
            ops.igemm(x, wp, M, K, N, out, res=u16, epilogue=ops.EPI_GELU_BWD, bf16=True, a16=True, o16=True, res16=True)
        return out, aux
    for form in ('f32res', 'drop', 'bf16', 'gelu16', 'dual16', 'dual32', 'gbwd'):
        prev = _lib.select(_lib.SEL_GEMM_TAIL, 1)                   # (off by default: faster alone, not in the timed steps)
        try:
            new, new_aux = run(form)
            _lib.select(_lib.SEL_GEMM_TAIL, 0)
            old, old_aux = run(form)
        finally:
            _lib.select(_lib.SEL_GEMM_TAIL, prev)
        assert not torch.isnan(new.float()).any() and not torch.isnan(old.float()).any(), form
        assert torch.equal(new, old), (form, (new.float() - old.float()).abs().max().item())
        if new_aux is not None:
            assert not torch.isnan(new_aux.float()).any() and torch.equal(new_aux, old_aux), form
    ref64 = x[-300:].double().cpu() @ _bf(w.cpu()) + b.double().cpu()                 # the last rows (tail tiles, ragged end) against fp64
    prev = _lib.select(_lib.SEL_GEMM_TAIL, 1)
    try:
        assert _rel(run('bf16')[0][-300:].float().cpu(), ref64) < 1e-2
    finally:
        _lib.select(_lib.SEL_GEMM_TAIL, prev)


@pytest.mark.parametrize('M,K,N', [(8192, 768, 1024), (1000, 768, 1024), (77, 128, 256)])
def test_fused_lmhead_argmax_equals_argmax_of_the_gemm_logits(dev, M, K, N):
    """vf_lmhead_argmax_bf16 (arg-max in the LM head's epilogue, logits never written) == vf_argmax_rows_f32(vf_gemm_bf16 logits), bit
    for bit: same packing, same k order, one fp32 chain per (row, code); fp32 and bf16 hidden rows; ties -> lowest index"""
    from viewformer_amd import ops
    wte = _rand((N + 2, K), 91, 0.05).to(dev)                         # [n_embeddings + 2][d] like the reference's wte (migt.py:288)
    wp = ops.pack_dense_nk_bf16(wte, n_rows=N)
    h = _rand((M, K), 92).to(dev)
    h[5] = h[4]                                                       # identical rows -> identical results
    logits = torch.empty((M, N), device=dev)
    ops.igemm(h, wp, M, K, N, logits, bf16=True)
    want = ops.argmax_rows(logits, M, N)
    got, mx = ops.lmhead_argmax_bf16(h, wp, M, K, N, want_max=True)
    assert torch.equal(got, want)
    assert torch.equal(mx, logits.gather(1, want.view(-1, 1)).view(-1))
    got16 = ops.lmhead_argmax_bf16(h.to(torch.bfloat16), wp, M, K, N)
    assert torch.equal(got16, want)                                   # bf16 rows = the rounding the kernel applies to fp32 rows
    # exact ties: duplicate codes -> the lowest index wins, as tf.argmax / vf_argmax_rows_f32
    if N > 900:
        wte2 = wte.clone()
        wte2[900] = wte2[17]
        g2 = ops.lmhead_argmax_bf16(h, ops.pack_dense_nk_bf16(wte2, n_rows=N), M, K, N)
        assert not (g2 == 900).any()
    assert not ops.lmhead_argmax_supported(768, 1000) and not ops.lmhead_argmax_supported(256, 1024)


def test_evaluator_with_fused_lmhead_is_bit_identical(dev, full_vq):
    """generate_batch_predictions without return_codes takes the fused LM-head arg-max; its images / cameras equal the logits path's"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.evaluate import generate_batch_predictions
    from viewformer_amd.migt import MIGT
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    vq_m = VQGAN(vcfg, data_format='NHWC', decoder_precision='bf16').load_state_dict(vsd).to(dev)
    frames, cams = synthetic_scene_batch(3, 4, 128, seed=5)
    for loc in ('1', '0'):
        mcfg = MIGTConfig(sequence_size=3, localization_weight=loc, pose_multiplier=0.2, n_layer=3)
        tr_m = MIGT(mcfg, precision='bf16').load_state_dict(make_migt_weights(mcfg, seed=2)).to(dev)
        a = generate_batch_predictions(tr_m, vq_m, frames, cams, return_codes=True)
        b = generate_batch_predictions(tr_m, vq_m, frames, cams)
        assert torch.equal(a['generated_images'], b['generated_images'])
        assert torch.equal(a['generated_cameras'], b['generated_cameras'])
        c = generate_batch_predictions(tr_m, vq_m, frames, cams, fused_passes=False)
        assert torch.equal(a['generated_images'], c['generated_images'])
