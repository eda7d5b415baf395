"""float64 restatement of the tree losses under label smoothing and probability targets, for the soft-target tests.

Built from nbdt.tree.FlatTree's CSR arrays with plain torch on the CPU: node logits as child means, per-node softmax,
the path product, then the criterion's formulas under autograd.  Not a product path and not the oracle: the tests pin it
to the reference's goldens (tests/golden/soft_targets_*.npz) and use it where no golden exists (other batch sizes).

  t'_c = (1 - eps)*t_c + eps/C,  T = sum_c t'_c      (torch does not normalise a probability row)
  soft row = w_x*(T*lse(z) - sum t'z) + w_t*(T*lse(P) - sum t'P)
  hard row = w_x*(lse(z) - (1-eps)*z_y - eps/C*sum z) + w_node * sum over the inner nodes n on y's path, K_n children,
             y under child s, of  lse(s_n) - (1-eps)*s_{n,s} - eps/K_n * sum_k s_{n,k}
  loss = mean of the rows
"""
import numpy as np
import torch


def _membership(flat):
    """[R, C] float64: slot s holds class c."""
    R, C = flat.num_slots, flat.num_classes
    M = torch.zeros(R, C, dtype=torch.float64)
    for s in range(R):
        M[s, torch.as_tensor(flat.slot_cls[flat.slot_off[s]:flat.slot_off[s + 1]].astype(np.int64))] = 1.0
    return M


def _node_logits(flat, z, M):
    return z @ (M / M.sum(1, keepdim=True)).T            # [B, R]: mean of the child's leaves


def soft_rules(flat, z):
    """Path probabilities P [B, C] (float64, differentiable) of logits z [B, C]."""
    M = _membership(flat)
    S = _node_logits(flat, z, M)
    logp = torch.cat([torch.log_softmax(S[:, flat.node_off[n]:flat.node_off[n + 1]], dim=1)
                      for n in range(flat.num_inodes)], dim=1)
    return torch.exp(logp @ M)


def smooth(t, eps):
    return (1.0 - eps) * t + eps / t.shape[1]


def soft_loss(flat, z, target, eps, w_xent, w_tree):
    """(loss, dloss/dz) as float64 numpy.  target: int64 [B] class indices or float [B, C] rows."""
    z = torch.as_tensor(np.asarray(z), dtype=torch.float64).clone().requires_grad_(True)
    target = torch.as_tensor(np.asarray(target))
    t = torch.nn.functional.one_hot(target, z.shape[1]).double() if target.dim() == 1 else target.double()
    t = smooth(t, eps)
    T = t.sum(1)
    P = soft_rules(flat, z)
    rows = w_xent * (T * torch.logsumexp(z, 1) - (t * z).sum(1)) + w_tree * (T * torch.logsumexp(P, 1) - (t * P).sum(1))
    loss = rows.mean()
    loss.backward()
    return loss.item(), z.grad.numpy()


def hard_loss(flat, z, y, eps, w_xent, w_node):
    """(loss, dloss/dz) as float64 numpy; y: int64 [B]."""
    z = torch.as_tensor(np.asarray(z), dtype=torch.float64).clone().requires_grad_(True)
    y = [int(v) for v in np.asarray(y)]
    M = _membership(flat)
    S = _node_logits(flat, z, M)
    C = z.shape[1]
    rows = []
    for b, yb in enumerate(y):
        row = w_xent * (torch.logsumexp(z[b], 0) - (1.0 - eps) * z[b, yb] - eps / C * z[b].sum())
        for n in range(flat.num_inodes):
            lo, hi = int(flat.node_off[n]), int(flat.node_off[n + 1])
            under = [s for s in range(lo, hi) if M[s, yb] > 0]
            if not under:
                continue
            s_n = S[b, lo:hi]
            row = row + w_node * (torch.logsumexp(s_n, 0) - (1.0 - eps) * S[b, under[0]] - eps / (hi - lo) * s_n.sum())
        rows.append(row)
    loss = torch.stack(rows).mean()
    loss.backward()
    return loss.item(), z.grad.numpy()
