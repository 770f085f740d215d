"""DAgger on one GPU: the learner acts in a DeviceNavEnv, a NavExpert labels every state it visits, a DemoPool
keeps (observation, label) rows, and GenericPPO.clone_actor fits the actor to them; afterwards the net goes to
runner/device_loop.train_states as it is.

Per step, all on the current stream and without a host synchronisation:
  net.forward on row set t of the pool (a sampled action)  ->  expert.mix (labels into row set t, the played action from the labels and
  the policy's by beta)  ->  env.step(played, obs_out = row set t + 1).
An observation and its label share a row.  No launch reads what another is writing: the launches of a step are ordered on one stream,
the forward reads row set t, the expert writes the labels of t and reads the env's state, and the step writes the state and renders
into row set t + 1, which nothing reads before the next step's forward; a pool has at least two row sets, so t and t + 1 never share
rows."""
import torch

from ddrl4nav_amd.data.demo_pool import same_device
from ddrl4nav_amd.nn.dagger import CloneTrainer


def default_betas(iterations):
    """1 for the first iteration -- the first data set is the expert's own trajectories -- then linearly down to 0 at the last."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError("iterations must be at least 1, got %d" % iterations)
    return [1.0] if iterations == 1 else [1.0 - i / (iterations - 1) for i in range(iterations)]


def _check(net, env, expert, pool):
    if expert.env is not env:
        raise ValueError("the expert reads another env")
    if pool.n_envs != env.N:
        raise ValueError("the pool advances %d rows a step, the env has %d" % (pool.n_envs, env.N))
    if [tuple(c.shape[1:]) for c in pool.components] != [tuple(s) for s in env.state_shapes]:
        raise ValueError("the pool's components %r are not the env's %r" % ([tuple(c.shape[1:]) for c in pool.components], env.state_shapes))
    if not net.continuous or net.n_actions != 2 or pool.action_dim != 2:
        raise ValueError("the navigation env takes the 2 actions of a Gaussian actor; the net has %d (%s), the pool %d"
                         % (net.n_actions, "Gaussian" if net.continuous else "Categorical", pool.action_dim))
    if not same_device(pool.device, env.device):
        raise ValueError("the pool lives on %s, the env on %s" % (pool.device, env.device))


def collect(net, env, expert, pool, steps, beta, step0=0, close=False, record=None):
    """`steps` steps of the loop above at mixing rate `beta`; the draws of the mixing are those of steps step0 .. step0 + steps - 1.
    The env must have been reset.  The last rendered observation waits in the pool for its label, which the next call writes first;
    close=True renders it into the env's own tensors instead, so that the pool ends without a waiting row (the next call copies it
    in).  record: a list that receives (policy action, played action) clones per step.  -> step0 + steps."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1, got %d" % steps)
    _check(net, env, expert, pool)
    if not pool.pending:
        comps, _ = pool.rows(pool.open())
        for dst, src in zip(comps, env.obs):
            dst.copy_(src)
    for s in range(steps):
        comps, labels = pool.rows(pool.cursor - 1)
        with torch.no_grad():
            (dist, _), _ = net.forward(comps)
        action = dist.sample()
        _, played = expert.mix(action, beta, (int(step0) + s) & 0xFFFFFFFF, labels_out=labels)
        pool.close_label()
        if record is not None:
            record.append((action.clone(), played.clone()))
        if close and s == steps - 1:
            env.step(played)
        else:
            env.step(played, obs_out=pool.rows(pool.open())[0])
    return int(step0) + steps


def run(net, env, expert, pool, iterations, steps, betas=None, lr=1e-4, batch=256, epochs=1, seed=0):
    """`iterations` rounds of collect(steps) and clone_actor(epochs) with one CloneTrainer (its Adam state persists over the rounds);
    yields (mean clone loss of the round, beta).  betas: one mixing rate per round (default_betas)."""
    betas = default_betas(iterations) if betas is None else [float(b) for b in betas]
    if len(betas) != int(iterations):
        raise ValueError("betas must name one rate per iteration: %d for %d" % (len(betas), int(iterations)))
    _check(net, env, expert, pool)
    trainer = CloneTrainer(net, pool, lr)
    step0 = 0
    for i, beta in enumerate(betas):
        step0 = collect(net, env, expert, pool, steps, beta, step0)
        log = net.clone_actor(pool, lr, batch, epochs, int(seed) + i, trainer=trainer)
        yield (sum(row[2] for row in log) / len(log) if log else float("nan")), beta
