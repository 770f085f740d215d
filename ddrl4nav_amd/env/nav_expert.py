"""NavExpert: the scripted expert of a DeviceNavEnv (csrc/navexpert.hip).

The reference's imitation start (MIMIC_START, Basenn.imitation_learning) needs demonstrations; its navigation task has none in the tree
(sh/start_dagger.sh is empty).  On the device env the expert may read the env's privileged state, so labelling every state a learner
visits -- DAgger -- costs one small launch per step: 51 constant-(v, w) arcs are rolled ten steps ahead against the wall, the obstacles
and the pedestrians' straight-line predictions, and the arc that gets nearest to the goal without a hit wins.  The rules are
integer-only (tests/nav_expert_ref.py is the rule book), so labels are reproducible bit for bit from the env's state.

The expert is the same under both pedestrian models of the env: it reads the state, which has the same words
under "walk" and "avoid", and predicts every pedestrian straight ahead at its current heading.  Under "avoid" that prediction is wrong
where a pedestrian turns away, which only adds margin; the expert's reach rate on the rule book's env is higher there (section 6.16)."""
import torch

from ddrl4nav_amd import ops
from ddrl4nav_amd.env.device_nav_env import DeviceNavEnv
from ddrl4nav_amd.env.fleet_nav_env import FleetNavEnv


class NavExpert:
    def __init__(self, env):
        """env: the DeviceNavEnv whose state the expert reads (never writes).  A FleetNavEnv is refused: its state layout and the
        robots' collisions with each other need rules of their own, which are not built."""
        if isinstance(env, FleetNavEnv):
            raise NotImplementedError("NavExpert is built for DeviceNavEnv only: a FleetNavEnv's state layout and its robot-robot "
                                      "collisions need rules of their own")
        if not isinstance(env, DeviceNavEnv):
            raise TypeError("NavExpert needs a DeviceNavEnv, got %r" % type(env))
        self.env = env
        self._labels = torch.empty((env.N, 2), dtype=torch.float32, device=env.device)
        self._played = torch.empty((env.N, 2), dtype=torch.float32, device=env.device)

    def _kw(self):
        e = self.env
        return dict(env0=e.env0, seed=e.seed, n_obstacles=e.n_obstacles, n_peds=e.n_peds)

    def labels(self, out=None):
        """The expert's action for the env's current state, fp32 [N, 2] = (v / 32, w / 64): what env.step decodes back to (v, w).  out:
        write there (contiguous fp32 [N, 2] on the env's device) instead of the expert's own tensor.  Asynchronous."""
        out = self._labels if out is None else out
        ops.nav_expert(self.env.state, label=out, **self._kw())
        return out

    def mix(self, policy_actions, beta, step, labels_out=None, played_out=None):
        """DAgger's mixed action: env i plays the expert's label where hash32(seed, global index of i, step) < floor(beta 2^32) and
        policy_actions[i] (fp32 [N, 2], bits kept) elsewhere; beta = 1 plays the expert, beta = 0 the policy.  The caller passes `step`
        (any counter that differs from step to step); the env's own event counter is not touched.  -> (labels, played), the expert's own
        tensors or labels_out / played_out.  Asynchronous."""
        labels = self._labels if labels_out is None else labels_out
        played = self._played if played_out is None else played_out
        ops.nav_expert(self.env.state, label=labels, played=played, policy=policy_actions, step=int(step) & 0xFFFFFFFF,
                       threshold=ops.beta_threshold(beta), **self._kw())
        return labels, played
