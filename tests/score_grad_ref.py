"""Shared by tests/test_score_grad_host.py and tests/test_hip_score_grad.py: the oracle's gradient of a photo's log-likelihood with respect
to the query camera, and a numpy brute force of ``render.ascend_poses``.  No device is needed to import or to run this."""
import numpy as np
import torch


def oracle_log_likelihood(sd, cfg, ctx_codes, ctx_poses, pose, codes, dtype):
    """sum over the tokens of log_softmax(logits of the MASK view)[code]: the oracle's full pass on [ctx, MASK] with poses [ctx, pose];
    ``ctx_codes`` [C,t,t], ``ctx_poses`` [C,7], ``pose`` [7], ``codes`` [t,t] -> 0-d tensor (with a graph where ``pose`` has one)"""
    from oracle import migt_oracle as mg
    ids = torch.cat([ctx_codes.long(), torch.full_like(ctx_codes[:1].long(), cfg.n_embeddings)], 0)[None]
    poses = torch.cat([ctx_poses.to(pose.dtype), pose[None]], 0)[None]
    lg = mg.migt_forward(sd, cfg, ids, poses, dtype=dtype, grad=pose.requires_grad)['logits'][0, -1]
    lp = torch.log_softmax(lg.reshape(-1, cfg.n_embeddings), -1)
    return lp.gather(1, codes.reshape(-1, 1).long()).sum()


def oracle_grad(sd, cfg, ctx_codes, ctx_poses, poses, codes, dtype=torch.float64):
    """d log_likelihood[n] / d poses[n] by autograd of the oracle, the 7 numbers free: ``poses`` [N,7], ``codes`` [N,t,t] ->
    (grad [N,7] float64, log_likelihood [N] float64).  The oracle carries the poses in float32 (as the model receives them) and
    computes in ``dtype``."""
    gs, lls = [], []
    for n in range(poses.shape[0]):
        p = poses[n].detach().clone().to(torch.float32).double().requires_grad_(True)       # a float64 leaf holding float32 values: p.grad is float64
        ll = oracle_log_likelihood(sd, cfg, ctx_codes, ctx_poses, p, codes[n], dtype)
        ll.backward()
        gs.append(p.grad.double())
        lls.append(ll.detach().double())
    return torch.stack(gs), torch.stack(lls)


def oracle_central_differences(sd, cfg, ctx_codes, ctx_poses, pose, codes, h=2.0 ** -9):
    """the same derivative by central differences of the float64 oracle, 14 forward passes; ``pose`` must be a multiple of ``h`` in every
    component so that pose +- h is exact in the float32 the oracle carries poses in"""
    g = torch.zeros(7, dtype=torch.float64)
    for i in range(7):
        e = torch.zeros(7, dtype=torch.float32)
        e[i] = h
        up = oracle_log_likelihood(sd, cfg, ctx_codes, ctx_poses, pose + e, codes, torch.float64)
        dn = oracle_log_likelihood(sd, cfg, ctx_codes, ctx_poses, pose - e, codes, torch.float64)
        g[i] = (up - dn) / (2 * h)
    return g


def ascend_brute(poses, grad, step_xyz, step_rot):
    """``render.ascend_poses`` pose by pose in numpy float64: [n,7] x 2, steps [n] -> [n,7]"""
    out = np.array(poses, dtype=np.float64)
    for i, (p, g) in enumerate(zip(np.asarray(poses, dtype=np.float64), np.asarray(grad, dtype=np.float64))):
        gx = g[:3]
        if np.linalg.norm(gx) > 0:
            out[i, :3] = p[:3] + step_xyz[i] * gx / np.linalg.norm(gx)
        q = p[3:] / np.linalg.norm(p[3:])
        t = g[3:] - np.dot(g[3:], q) * q
        if np.linalg.norm(t) > 1e-6 * np.linalg.norm(g[3:]):             # (a purely radial g_q is no direction)
            q2 = q + step_rot[i] * t / np.linalg.norm(t)
            q2 = q2 / np.linalg.norm(q2)
            out[i, 3:] = q2 if q2[0] >= 0 else -q2
    return out
