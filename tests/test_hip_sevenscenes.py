"""GPU: the scene bank and the 7-Scenes generation procedures (viewformer_amd/scene_bank.py, evaluate_sevenscenes.py) stage by stage:
every stage is judged on the GPU path's own inputs to it, so that an allowed 1e-3 upstream cannot become an index flip downstream.
Full-size VQGAN, a 4-layer MIGT (as tests/test_hip_models.py::test_generate_batch_predictions_matches_oracle), a bank of 40 synthetic
frames, sequences of 5 views.  Bounds are that test's: logits 1e-3, generated-code agreement > 0.97, cameras 1e-3.
Measured on an MI355X: first-pass camera 9e-6 / 1e-5 (B = 1 / 3); refined pass against the pipeline oracle: logits 8e-5 / 1e-4, cameras
1e-5 / 6e-5, code agreement 1.0; generated_images' four passes 3.7e-4, 9.1e-5, 7.8e-5, 2.7e-4, code agreement 1.0."""
import random

import numpy as np
import pytest
import torch

import sevenscenes_ref as ref

pytestmark = pytest.mark.gpu

CTX = 4                # context views per query (the reference: 19)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def world(dev, full_vq):
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.scene_bank import SceneBank
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    mcfg = MIGTConfig(sequence_size=CTX + 1, localization_weight='1', pose_multiplier=0.2, n_layer=4)
    msd = make_migt_weights(mcfg, seed=1, std=0.05)
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x6').load_state_dict(vsd).to(dev)
    tr_m = MIGT(mcfg).load_state_dict(msd).to(dev)
    frames, cams = synthetic_scene_batch(1, 40, 128, seed=21)
    bank = SceneBank(vq_m, torch.from_numpy(frames[0]), cams[0], batch_size=16)          # chunks of 16, 16 and 8 frames
    return dict(vcfg=vcfg, vsd=vsd, mcfg=mcfg, msd=msd, vq=vq_m, tr=tr_m, bank=bank, frames=torch.from_numpy(frames[0]), cams=cams[0])


def _maxerr(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


def _queries(world, B, seed=22):
    """B queries with their drawn context: (frames [B,S,H,W,3], cameras [B,S,7], context indices [B,S-1])"""
    from viewformer_amd.evaluate_sevenscenes import build_batch
    from viewformer_amd.weights import synthetic_scene_batch
    qf, qc = synthetic_scene_batch(B, 1, 128, seed=seed)
    built = [build_batch(world['bank'], torch.from_numpy(qf[b]), qc[b], context_size=CTX, rng=random.Random(40 + b)) for b in range(B)]
    return torch.cat([x[1] for x in built]), torch.cat([x[0] for x in built]), [x[2] for x in built]


def test_scene_bank_codes_are_the_encoders(dev, world):
    from viewformer_amd import ops
    bank, vq_m = world['bank'], world['vq']
    assert len(bank) == 40 and tuple(bank.codes.shape) == (40, 8, 8) and bank.codes.dtype == torch.int32
    assert tuple(bank.cameras.shape) == (40, 7) and bank.cameras.dtype == torch.float32 and bank.cameras.is_cuda
    sel = torch.tensor([0, 15, 16, 17, 31, 32, 39, 5])
    direct = vq_m.encode(world['frames'][sel].to(dev))[-1]
    assert torch.equal(bank.codes[sel.to(dev)], direct.to(torch.int32))                    # bit for bit across the chunk boundaries
    cam, i = bank['frame-000017.color.png']
    assert i == 17 and bank.index('frame-000017.color.png') == 17 and np.array_equal(cam, world['cams'][17])
    idx = torch.tensor([[3, 1, 39], [0, 0, 7]])
    codes, cams = bank.gather(idx)
    assert torch.equal(codes, bank.codes[idx.to(dev)]) and tuple(codes.shape) == (2, 3, 8, 8)
    assert torch.equal(cams.cpu(), torch.from_numpy(world['cams'])[idx])
    assert torch.equal(bank.frames_at(idx).cpu(), world['frames'][idx])
    q = torch.from_numpy(ref.cameras('free', 3, 1)).to(dev)
    assert torch.equal(bank.nearest(q, 5), ops.camera_knn(bank.cameras, q, 5, 0.3))
    # a bank of larger frames resizes as the evaluators do
    from viewformer_amd.scene_bank import SceneBank
    big = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(3, 160, 160, 3), dtype=np.uint8))
    b2 = SceneBank(vq_m, big, world['cams'][:3], files=['a', 'b', 'c'], batch_size=2, keep_frames=False)
    assert torch.equal(b2.codes, vq_m.encode(ops.resize_u8(big.to(dev), 128))[-1].to(torch.int32)) and b2.index('c') == 2
    with pytest.raises(RuntimeError):
        b2.frames_at(idx)


@pytest.mark.parametrize('B', [1, 3])
def test_pose_refinement_stage_by_stage(dev, world, B):
    from oracle import migt_oracle as mg
    from oracle import pipeline_oracle as po
    from viewformer_amd import evaluate
    from viewformer_amd.evaluate_sevenscenes import generate_batch_predictions_using_pose_refinement as refine
    bank, vq_m, tr_m, mcfg, msd = world['bank'], world['vq'], world['tr'], world['mcfg'], world['msd']
    frames, cams, indices = _queries(world, B)
    fill = [[3 + b, 20 + b] for b in range(B)]
    got = refine(bank, tr_m, vq_m, frames, cams, num_gen_ctx=2, fill_indices=fill, context_size=CTX, context_indices=indices,
                 return_intermediates=True)
    torch.cuda.synchronize()
    # the context codes came from the bank; the query's from the encoder
    assert torch.equal(got['first_pass_codes'][:, :-1], bank.codes[torch.tensor(indices).to(dev)])
    assert torch.equal(got['first_pass_codes'][:, -1], vq_m.encode(frames[:, -1].to(dev))[-1].to(torch.int32))
    # (a) the first-pass camera against the oracle fed the same codes
    rel, transform = mg.to_relative_cameras(cams)
    rel = mg.normalize_cameras(rel)
    out = mg.migt_forward(msd, mcfg, got['first_pass_codes'].cpu(), rel[:, :-1], dtype=torch.float64)
    want_cam = mg.from_relative_cameras(mg.reduce_cameras(out['pose_prediction'][:, -1:].to(torch.float32), -2), transform)[:, 0]
    e_a = _maxerr(got['first_pass_camera'], want_cam)
    # (b) the reported neighbours against the fp64 argsort AT the reported camera
    first = got['first_pass_camera'].cpu().numpy()
    d64 = ref.distances64(world['cams'], first)
    tol = ref.tolerance(world['cams'], first, 2, d64)
    gaps = np.diff(np.sort(d64, -1)[:, :3], axis=-1)
    print(f'B={B}: first-pass camera error {e_a:.2e}; knn tol {tol:.2e}, smallest gap among the first 3 distances {gaps.min():.2e}')
    assert e_a < 1e-3
    assert (gaps > 2 * tol).all()                                                          # 40 cameras: no near-ties to exempt
    assert np.array_equal(got['nearest'].cpu().numpy(), ref.top_rows(d64, 2))
    assert torch.equal(got['context_indices'].cpu(), torch.cat((got['nearest'].cpu(), torch.tensor(fill, dtype=torch.int32)), 1))
    # (c) == the standard evaluator on the frames those indices name: through reencode=True and through a direct call
    ctx = got['context_indices'].cpu().long()
    named_frames = torch.cat((world['frames'][ctx], frames[:, -1:]), 1)
    named_cams = torch.cat((torch.from_numpy(world['cams'])[ctx], cams[:, -1:]), 1)
    direct = evaluate.generate_batch_predictions(tr_m, vq_m, named_frames, named_cams, return_codes=True)
    again = refine(bank, tr_m, vq_m, frames, cams, num_gen_ctx=2, fill_indices=fill, context_size=CTX, reencode=True,
                   return_intermediates=True)
    for other in (direct, again):
        for k in ('generated_images', 'generated_cameras', 'ground_truth_images', 'ground_truth_cameras', 'codes', 'logits_last',
                  'generated_codes'):
            assert torch.equal(got[k], other[k]), k
    assert torch.equal(got['nearest'], again['nearest']) and torch.equal(got['first_pass_camera'], again['first_pass_camera'])
    # without the intermediates: the same predictions, and only the evaluator's keys
    plain = refine(bank, tr_m, vq_m, frames[:, -1:], cams, num_gen_ctx=2, fill_indices=fill, context_size=CTX, context_indices=indices)
    assert sorted(plain) == ['generated_cameras', 'generated_images', 'ground_truth_cameras', 'ground_truth_images']
    assert torch.equal(plain['generated_images'], got['generated_images']) and torch.equal(plain['generated_cameras'], got['generated_cameras'])
    # (d) that result against the pipeline oracle on those frames
    want = po.generate_batch_predictions(msd, mcfg, world['vsd'], world['vcfg'], named_frames, named_cams, return_intermediates=True)
    assert torch.equal(got['codes'].cpu(), want['codes'])
    e_l, e_c = _maxerr(got['logits_last'], want['logits_last']), _maxerr(got['generated_cameras'], want['generated_cameras'])
    same = (got['generated_codes'].cpu() == want['generated_codes']).float().mean().item()
    print(f'B={B}: refined pass vs pipeline oracle: logits {e_l:.2e}, cameras {e_c:.2e}, generated-code agreement {same:.3f}')
    assert e_l < 1e-3 and e_c < 1e-3 and same > 0.97
    # B queries in one call == B calls of one query, bit for bit
    if B > 1:
        for b in range(B):
            one = refine(bank, tr_m, vq_m, frames[b:b + 1], cams[b:b + 1], num_gen_ctx=2, fill_indices=fill[b:b + 1], context_size=CTX,
                         context_indices=indices[b:b + 1], return_intermediates=True)
            for k in ('generated_images', 'generated_cameras', 'first_pass_camera', 'nearest', 'logits_last'):
                assert torch.equal(one[k], got[k][b:b + 1]), (b, k)


def test_generated_images_pass_by_pass(dev, world):
    from oracle import migt_oracle as mg
    from viewformer_amd.evaluate_sevenscenes import (default_uniforms, generate_batch_predictions_using_generated_images as gen_images,
                                                     generate_other_viewpoints)
    from viewformer_amd import geometry
    vq_m, tr_m, mcfg, msd = world['vq'], world['tr'], world['mcfg'], world['msd']
    B, n, S = 2, 2, CTX + 1
    frames, cams, _ = _queries(world, B, seed=23)
    got = gen_images(tr_m, vq_m, frames, cams, num_gen_ctx=n, seed=[5, 6], return_intermediates=True)
    torch.cuda.synchronize()
    g = {k: v.cpu() for k, v in got.items()}
    rel = mg.normalize_cameras(mg.to_relative_cameras(cams)[0])
    assert _maxerr(g['cameras'], rel) < 1e-6
    assert torch.equal(got['codes'], vq_m.encode(frames.reshape(B * S, 128, 128, 3).to(dev))[-1].to(torch.int32).view(B, S, 8, 8))
    mask = torch.full_like(g['codes'][:, :1], mcfg.n_embeddings)

    def fwd(ids, poses):
        return mg.migt_forward(msd, mcfg, ids, poses, dtype=torch.float64)
    # pass 1: localization of the given views
    e1 = _maxerr(g['first_pass_pose'], fwd(g['codes'], g['cameras'][:, :-1])['pose_prediction'][:, -1:])
    assert torch.equal(got['first_pass_camera'], tr_m.reduce_cameras(got['first_pass_pose'], -2)[:, -1])
    # the perturbed cameras: the host restatement applied per scene to the GPU path's first-pass camera, draws of that scene's seed
    for b, seed in enumerate((5, 6)):
        want = geometry.normalize_cameras(generate_other_viewpoints(g['first_pass_camera'][b].view(1, 1, 7).repeat(n, 1, 1),
                                                                    default_uniforms((n, 1), seed)))
        assert _maxerr(g['new_cameras'][b], want) < 1e-6
    # pass 2: n generations per scene from the perturbed cameras
    assert torch.equal(g['pass2_input_ids'], torch.cat([g['codes'][:, :-1], mask], 1)[:, None].repeat(1, n, 1, 1, 1))
    assert torch.equal(g['pass2_poses'][:, :, :-1], g['cameras'][:, None, :-1].repeat(1, n, 1, 1))
    assert torch.equal(g['pass2_poses'][:, :, -1:], g['new_cameras'])
    e2, agree2 = 0.0, []
    for b in range(B):
        lg = fwd(g['pass2_input_ids'][b], g['pass2_poses'][b])['logits'][:, -1]
        e2 = max(e2, _maxerr(g['pass2_logits_last'][b], lg))
        agree2.append((g['new_codes'][b].long() == lg.argmax(-1)).float().mean().item())
        assert torch.equal(g['new_codes'][b].long(), g['pass2_logits_last'][b].argmax(-1))
    # the final sequence, literally (:120-127): the LAST n views — the target among them — are the generated ones
    assert torch.equal(g['final_codes'][:, :S - n], g['codes'][:, :S - n]) and torch.equal(g['final_codes'][:, S - n:], g['new_codes'])
    assert torch.equal(g['final_cameras'][:, :S - n], g['cameras'][:, :S - n])
    assert torch.equal(g['final_cameras'][:, S - n:], g['new_cameras'].reshape(B, n, 7))
    # pass 3 (generation) and pass 4 (localization) on that sequence
    lg3 = fwd(torch.cat([g['final_codes'][:, :-1], mask], 1), g['final_cameras'])['logits'][:, -1]
    e3 = _maxerr(g['logits_last'], lg3)
    agree3 = (g['generated_codes'].long() == lg3.argmax(-1)).float().mean().item()
    e4 = _maxerr(g['pose_last'], fwd(g['final_codes'], g['final_cameras'][:, :-1])['pose_prediction'][:, -1:])
    print(f'generated_images: pass errors {e1:.2e} {e2:.2e} {e3:.2e} {e4:.2e}; code agreement pass 2 {min(agree2):.3f}, pass 3 {agree3:.3f}')
    assert max(e1, e2, e3, e4) < 1e-3 and min(agree2) > 0.97 and agree3 > 0.97
    assert got['generated_images'].dtype == torch.uint8 and tuple(got['generated_images'].shape) == (B, 128, 128, 3)
    assert torch.equal(g['ground_truth_images'], frames[:, -1]) and torch.equal(g['ground_truth_cameras'], cams[:, -1])
    assert tuple(got['generated_cameras'].shape) == (B, 7)
    # the fused last pair == the reference's two separate passes, bit for bit
    sep = gen_images(tr_m, vq_m, frames, cams, num_gen_ctx=n, seed=[5, 6], return_intermediates=True, fused_passes=False)
    for k in ('logits_last', 'pose_last', 'generated_images', 'generated_cameras'):
        assert torch.equal(got[k], sep[k]), k
    # a fixed seed reproduces; another seed perturbs differently; the plain call gives the same predictions; scenes do not see each other
    plain = gen_images(tr_m, vq_m, frames, cams, num_gen_ctx=n, seed=[5, 6])
    assert sorted(plain) == ['generated_cameras', 'generated_images', 'ground_truth_cameras', 'ground_truth_images']
    assert torch.equal(plain['generated_images'], got['generated_images']) and torch.equal(plain['generated_cameras'], got['generated_cameras'])
    other = gen_images(tr_m, vq_m, frames, cams, num_gen_ctx=n, seed=7, return_intermediates=True)
    assert not torch.equal(other['new_cameras'], got['new_cameras'])
    for b, seed in enumerate((5, 6)):
        one = gen_images(tr_m, vq_m, frames[b:b + 1], cams[b:b + 1], num_gen_ctx=n, seed=seed)
        assert torch.equal(one['generated_images'], got['generated_images'][b:b + 1])
        assert torch.equal(one['generated_cameras'], got['generated_cameras'][b:b + 1])


@pytest.mark.parametrize('procedure', ['standard', 'generated_images', 'pose_refinement'])
def test_evaluate_scene_keys_and_batch_size_independence(dev, world, procedure):
    from viewformer_amd.evaluate_sevenscenes import evaluate_scene
    from viewformer_amd.weights import synthetic_scene_batch
    qf, qc = synthetic_scene_batch(6, 1, 128, seed=24)
    queries = [(torch.from_numpy(qf[i]), qc[i], f'seq-03/frame-{i:06d}') for i in range(6)]
    match_map = {f'seq-03/frame-{i:06d}.color.png': [world['bank'].files[(7 * i + j) % 40] for j in range(3)] for i in range(6)}
    runs = {}
    for bs in (1, 4):
        preds = []
        res = evaluate_scene(world['bank'], world['tr'], world['vq'], iter(queries), generation_procedure=procedure, num_gen_ctx=2,
                             batch_size=bs, match_map=match_map, top_n_matched_images=2, context_size=CTX, seed=3,
                             store_predictions=lambda **p: preds.append(p))
        assert list(res) == ['loc-angle', 'loc-dist', 'loc-angle-med', 'loc-dist-med', 'mse', 'rmse', 'mae', 'psnr', 'ssim']
        assert all(np.isfinite(v) for v in res.values())
        runs[bs] = (res, {k: torch.cat([p[k] for p in preds]) for k in preds[0]})
        assert [len(p['generated_images']) for p in preds] == ([1] * 6 if bs == 1 else [4, 2])
    for k, v in runs[1][1].items():
        assert torch.equal(v, runs[4][1][k]), k
    assert runs[1][0] == pytest.approx(runs[4][0], rel=1e-9)          # (the evaluator adds per batch: another order of the same sums)
    assert torch.equal(runs[1][1]['ground_truth_images'].cpu(), torch.from_numpy(qf[:, 0]))


def test_evaluate_scene_multictx(dev, world):
    from viewformer_amd.evaluate_sevenscenes import evaluate_scene_multictx
    from viewformer_amd.weights import synthetic_scene_batch
    qf, qc = synthetic_scene_batch(3, 1, 128, seed=25)
    queries = [(torch.from_numpy(qf[i]), qc[i], f'q{i}') for i in range(3)]
    res = evaluate_scene_multictx(world['bank'], world['tr'], world['vq'], queries, batch_size=2, context_size=CTX, seed=1)
    assert list(res) == [f'ctx{i:02d}' for i in range(1, CTX + 1)]
    keys = ['loc-angle', 'loc-dist', 'loc-angle-med', 'loc-dist-med', 'mse', 'rmse', 'mae', 'psnr', 'ssim']
    assert all(list(v) == keys and all(np.isfinite(x) for x in v.values()) for v in res.values())
