"""time a camera path whose frames agree with each other — frame t generated from the photographs AND the frames 0 ... t-1
(viewformer_amd/render.py) — three ways:
  (a) what a user does without a cache that grows: per step ``set_context(all views so far)`` + ``render`` of 1 view (the context's codes
      are encoded once beforehand and the generated code maps are fed back as codes: no encoder pass inside the loop);
  (b) one ``set_context`` + ``rollout(fused_step=False)``: per step a MASK pass and an append pass of 1 view each;
  (c) one ``set_context`` + ``rollout()``: per step ONE pass over 2 views per scene.
Full-size models of bench.py, both arms ('mixed': bf16 transformer and decoder; 'f32'), (C0, T, B) = (3, 16, 1), (3, 16, 16), (6, 32, 1).
The three routes' pictures are compared first: equal wherever their code maps agree, and the maps that agree are counted (the routes'
row counts differ, so a near-tie token may flip and the rest of that path with it).  In ONE process, the routes taking turns, every route
warmed first, device events around calls that end in a synchronise, windows of at least 0.4 s; median, min and max of the windows.  Next
to the times: the prefilled (context or appended) views each route runs, counted from the shapes, and the interval between back-to-back
``vf_kv_append`` launches as issued from Python at the shape's size (K = 1: an append pass, K = 2: the fused step) on the roll-out's own
buffers — 200 launches between two events, so the figure holds the host's submission interval and is an UPPER BOUND on the kernel's time.  Plain lines, then
one JSON line; the same text goes to ``--out`` (default profiles/rollout.txt)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import build_models                                                                     # noqa: E402
from viewformer_amd import ops                                                                      # noqa: E402
from viewformer_amd.evaluate import _frames_for_encode                                              # noqa: E402
from viewformer_amd.render import ViewRenderer                                                      # noqa: E402
from viewformer_amd.weights import synthetic_scene_batch                                            # noqa: E402

SHAPES = [(3, 16, 1), (3, 16, 16), (6, 32, 1)]
MIN_WINDOW_MS = 400.0
WINDOWS = 5
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, windows=WINDOWS):
    """{name: [ms per call, one figure per window]}: every candidate is warmed, sized to MIN_WINDOW_MS per window, and the candidates take turns"""
    calls = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        one = window_ms(fn, 1)
        calls[k] = max(1, int(MIN_WINDOW_MS / max(one, 1e-3)) + 1)
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, calls[k]))
    return out, calls


def summary(ms, calls):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), windows=len(ms), calls_per_window=calls)


def kv_append_us(r, B, K, launches=200):
    """vf_kv_append of K views per scene on layer 0's buffer of the renderer's cache, ``launches`` times back to back between two events:
    microseconds per launch AS ISSUED FROM PYTHON (ctypes call and submission included: an upper bound on the kernel's own time)"""
    cache = r.cache
    d = cache.kv[0].shape[1] // 3
    src = torch.zeros((B * K * 64, 3 * d), dtype=cache.kv[0].dtype, device=cache.kv[0].device)
    pos = torch.full((B,), cache.capacity - K, dtype=torch.int32, device=src.device)              # the last K views of room
    fn = lambda: ops.kv_append(src, cache.kv[0], B, K, 64, d, 3 * d, 3 * d, cache.capacity * 64 * 3 * d, cache.capacity, pos)
    fn()
    torch.cuda.synchronize()
    ms = sorted(window_ms(fn, launches) for _ in range(5))
    return round(ms[2] * 1e3, 2), round(2 * B * K * 64 * d * src.element_size() / 1e6, 3)          # median, MB each way


def run_shape(dev, arm, vq, tr, C0, T, B, windows=WINDOWS):
    frames, cams = synthetic_scene_batch(B, C0 + T, 128, seed=7)
    frames, cams = torch.from_numpy(frames).to(dev), torch.from_numpy(cams).to(dev)
    ctx_c, path = cams[:, :C0].contiguous(), cams[:, C0:].contiguous()
    t = tr.config.token_image_size
    codes = vq.encode(_frames_for_encode(frames[:, :C0].contiguous(), vq.config.image_size))[-1].to(torch.int32).view(B, C0, t, t)
    keep = {}

    def per_step(want_codes=False):
        seq, imgs = codes, []
        for s in range(T):
            out = ViewRenderer(tr, vq).set_context(codes=seq, cameras=cams[:, :C0 + s]).render(path[:, s:s + 1], return_codes=True)
            seq = torch.cat([seq, out['generated_codes'].to(torch.int32)], 1)
            imgs.append(out['generated_images'])
        keep['a'] = torch.cat(imgs, 1)
        keep['a_codes'] = seq[:, C0:]

    def rollout(name, **kw):
        def fn(want_codes=False):
            out = ViewRenderer(tr, vq).set_context(codes=codes, cameras=ctx_c, capacity=C0 + T).rollout(path, return_codes=want_codes, **kw)
            keep[name] = out['generated_images']
            if want_codes:
                keep[name + '_codes'] = out['generated_codes']
        return fn
    two_pass, fused = rollout('b', fused_step=False), rollout('c', fused_step=True)
    # the three routes' results first: equal pictures wherever the code maps agree
    per_step()
    two_pass(True)
    fused(True)
    agree = {}
    for x in ('b', 'c'):
        same = (keep['a_codes'].long() == keep[x + '_codes']).flatten(2).all(-1)                   # [B,T]
        assert torch.equal(keep['a'][same], keep[x][same]), f'({x}) and (a) decode equal code maps to different pictures'
        agree[x] = int(same.sum())
    same_bc = (keep['b_codes'] == keep['c_codes']).flatten(2).all(-1)
    assert torch.equal(keep['b'][same_bc], keep['c'][same_bc])
    t_ms, calls = alternate(dict(per_step=per_step, two_pass=two_pass, fused=fused), windows)
    res = {k: summary(v, calls[k]) for k, v in t_ms.items()}
    res['a_over_c'] = round(res['per_step']['median_ms'] / res['fused']['median_ms'], 2)
    res['b_over_c'] = round(res['two_pass']['median_ms'] / res['fused']['median_ms'], 3)
    res['prefilled_views'] = dict(per_step=B * sum(C0 + s for s in range(T)), two_pass=B * (C0 + T), fused=B * (C0 + T))
    res['maps'] = B * T
    res['maps_agreeing'] = dict(b_with_a=agree['b'], c_with_a=agree['c'], c_with_b=int(same_bc.sum()))
    r = ViewRenderer(tr, vq).set_context(codes=codes, cameras=ctx_c, capacity=C0 + T)
    res['kv_append_us'] = {f'K{K}': dict(zip(('us_per_launch', 'MB_each_way'), kv_append_us(r, B, K))) for K in (1, 2)}
    m = lambda k: res[k]['median_ms']
    say(f'{arm:5s} C0={C0} T={T:2d} B={B:2d}: (a) per step {m("per_step"):9.2f} ms  (b) two passes {m("two_pass"):9.2f} ms  (c) fused step {m("fused"):9.2f} ms  '
        f'(a)/(c) x{res["a_over_c"]}  (b)/(c) x{res["b_over_c"]}')
    say('      spread [min..max] ' + '  '.join(f'{k} {res[k]["min_ms"]}..{res[k]["max_ms"]} ({calls[k]} calls)' for k in t_ms) + f'  ({windows} windows)')
    pv, ag, ka = res['prefilled_views'], res['maps_agreeing'], res['kv_append_us']
    say(f'      prefilled views (a) {pv["per_step"]}  (b) {pv["two_pass"]}  (c) {pv["fused"]};  code maps of {B * T} agreeing: (b) with (a) {ag["b_with_a"]}, '
        f'(c) with (a) {ag["c_with_a"]}, (c) with (b) {ag["c_with_b"]} (pictures equal on all of them);  vf_kv_append per back-to-back launch as issued from Python: '
        f'K=1 {ka["K1"]["us_per_launch"]} us ({ka["K1"]["MB_each_way"]} MB each way), K=2 {ka["K2"]["us_per_launch"]} us ({ka["K2"]["MB_each_way"]} MB)')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'rollout.txt'))
    ap.add_argument('--windows', type=int, default=WINDOWS)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    out = {}
    say(f'roll-out along a camera path, {torch.cuda.get_device_name(0)}: ms per path, median of {args.windows} windows >= {MIN_WINDOW_MS:.0f} ms, routes alternating')
    for arm in ('mixed', 'f32'):
        vq, tr, _ = build_models(dev, False, arm, 'x3h', sequence_size=max(c + t for c, t, _ in SHAPES) + 1)
        for C0, T, B in SHAPES:
            out[f'{arm}_C{C0}_T{T}_B{B}'] = run_shape(dev, arm, vq, tr, C0, T, B, args.windows)
        del vq, tr
        torch.cuda.empty_cache()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(_lines) + '\n')


if __name__ == '__main__':
    main()
