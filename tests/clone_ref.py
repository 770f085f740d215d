"""The float64 statement of one clone step (ddrl4nav_amd/nn/dagger.py) on cells of tests/generic_cross.py: the
actor side of the oracle net alone -- its encoder and actor_linear -- under mean((mu - y)^2) / 2 (Gaussian) or F.cross_entropy
(Categorical), then autograd.  No GPU: tests/test_clone_cpu.py holds the statement's fp32 form to half the GPU bound on these cells."""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import generic_cross as X

# net / head, batch (n, max_batch); the knobs of a PPO update play no part in a clone step
CELLS = [
    X.Cell("mlp_split", "gauss3", 0, "default", "none", 0, 37, 37),
    X.Cell("mlp_shared", "cat5", 0, "default", "none", 0, 37, 37),
    X.Cell("nav1d_split", "gauss1", 0, "default", "none", 0, 37, 37),
    X.Cell("navped_shared", "cat9", 0, "default", "none", 0, 37, 37),
    X.Cell("mlp_split", "gauss1", 0, "default", "none", 0, 7, 3),       # micro-batches of 3, 3 and 1 folded into one gradient
]
LR = 3e-4
GRAD_BOUND = 2e-5          # per tensor, of max|want| (tests/test_generic_cross_gpu.py)
LOSS_RTOL = 2e-5

Clone = namedtuple("Clone", "loss metric grads mu")


def cell_id(cell):
    return "%s-%s-n%d-mb%d" % (cell.net, cell.head, cell.n, cell.max_batch)


@functools.lru_cache(maxsize=None)
def labels_of(cell):
    """Demonstrated actions float32 [n, D] (Gaussian: N(0, 0.5)) or action indices float32 [n, 1] (Categorical), seeded by the cell."""
    rng = np.random.RandomState(X.cell_seed(cell) % (2 ** 31))
    if X.gaussian(cell):
        return (0.5 * rng.normal(size=(cell.n, X.n_out(cell)))).astype(np.float32)
    return rng.randint(0, X.n_out(cell), size=(cell.n, 1)).astype(np.float32)


def actor_side(cell):
    """The parameter-name prefixes a clone step gives a gradient: the actor's encoder and actor_linear."""
    return ("prenet.", "actor.actor_linear.") if X.shared(cell) else ("actor.pre.", "actor.actor_linear.")


def clone_statement(cell, x, labels, dtype=torch.float64, sub=None, record=None, weights=None):
    """One loss + backward of the actor side in `dtype`.  sub / record: the dicts of oracle_nav._act for the actor's encoder.
    -> Clone(loss, metric, {name: gradient or None}, mu or logits)."""
    net = X.oracle_net(cell, x.weights if weights is None else weights, dtype)
    enc = X.encoders(net)[0]
    if sub is not None:
        enc.sub = sub
    if record is not None:
        enc.record = record
    st = [torch.from_numpy(s).to(dtype) for s in x.states]
    y = torch.from_numpy(np.asarray(labels)).to(dtype)
    out = net.actor.actor_linear(enc(st))
    if X.gaussian(cell):
        loss = torch.mean((out - y) ** 2) / 2
        metric = float((out - y).detach().abs().sum())
    else:
        loss = F.cross_entropy(out, y.reshape(-1).long())
        metric = float((out.argmax(1) == y.reshape(-1).long()).sum())
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().double().numpy()) for k, p in net.named_parameters()}
    return Clone(loss.item(), metric, grads, out.detach().double().numpy())


def fp32_decisions(cell, x, labels):
    """{site: ReLU output} of the fp32 statement's own forward: the decisions both precisions are then compared under."""
    rec = {}
    clone_statement(cell, x, labels, torch.float32, record=rec)
    return X.relu_of(rec)
