"""What DeviceEnv (env/device_env.py) and DeviceNavEnv (env/device_nav_env.py) share: the checks of n_envs / seed / env0, the state,
reward and done tensors, and the checkpoint of the state words next to the parameters a subclass names in _PARAMS.  FleetNavEnv
(env/fleet_nav_env.py), whose state has a row per world and whose outputs have a row per robot, allocates for itself and shares the
checkpoint."""
import torch


class DeviceEnvBase:
    _PARAMS = ()              # the constructor arguments (attributes of the same name) a saved env has to agree on
    _state_ints = None        # the int32 words of one env's state: a callable of the library

    def __init__(self, n_envs, device, seed, env0):
        """After the subclass's own checks: nothing is allocated for a refused argument."""
        self.N, self.seed, self.env0 = int(n_envs), int(seed), int(env0)
        if self.N < 1:
            raise ValueError("n_envs must be at least 1, got %d" % self.N)
        if not 0 <= self.seed < 2 ** 32:
            raise ValueError("seed must fit 32 bits, got %d" % self.seed)
        if self.env0 < 0 or self.env0 + self.N > 2 ** 32:
            raise ValueError("global env indices env0 .. env0 + n_envs - 1 must fit 32 bits")
        self.device = dev = torch.device("cuda" if device is None else device)
        self.state = torch.zeros((self.N, self._state_ints()), dtype=torch.int32, device=dev)
        self.reward = torch.zeros(self.N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(self.N, dtype=torch.uint8, device=dev)

    @property
    def n_envs(self):
        return self.N

    def state_dict(self):
        """The state words (a host tensor) and the parameters: an env loaded from it continues bit-identically."""
        sd = {k: getattr(self, k) for k in self._PARAMS}
        sd["state"] = self.state.cpu()
        return sd

    def load_state_dict(self, sd):
        for k in self._PARAMS:
            if sd[k] != getattr(self, k):
                raise ValueError("%s differs between the saved env (%r) and this one (%r)" % (k, sd[k], getattr(self, k)))
        s = torch.as_tensor(sd["state"])
        if s.dtype != torch.int32 or tuple(s.shape) != tuple(self.state.shape):
            raise ValueError("state must be int32 %s, got %s %s" % (tuple(self.state.shape), s.dtype, tuple(s.shape)))
        self.state.copy_(s)
