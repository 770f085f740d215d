"""What DeviceEnv (env/device_env.py), DeviceNavEnv (env/device_nav_env.py) and FleetNavEnv (env/fleet_nav_env.py) share: the checks of the
population / seed / first global index, the state, reward and done tensors, and the checkpoint of the state words next to the parameters
a subclass names in _PARAMS.  A state row may own several output rows (rows_per_state: FleetNavEnv's world and its robots); ``N`` counts
the output rows, which is what everything downstream of an env works on."""
import torch


class DeviceEnvBase:
    _PARAMS = ()              # the constructor arguments (attributes of the same name) a saved env has to agree on
    _state_ints = None        # the int32 words of one state row: a callable of the library

    def __init__(self, n_envs, device, seed, env0, rows_per_state=1):
        """After the subclass's own checks: nothing is allocated for a refused argument.  n_envs counts the state rows and env0 is the
        global index of the first (FleetNavEnv: its worlds and world0, which it checks under those names first)."""
        n, self.seed, self.env0 = int(n_envs), int(seed), int(env0)
        if n < 1:
            raise ValueError("n_envs must be at least 1, got %d" % n)
        if not 0 <= self.seed < 2 ** 32:
            raise ValueError("seed must fit 32 bits, got %d" % self.seed)
        if self.env0 < 0 or self.env0 + n > 2 ** 32:
            raise ValueError("global env indices env0 .. env0 + n_envs - 1 must fit 32 bits")
        self.N = n * int(rows_per_state)
        self.device = dev = torch.device("cuda" if device is None else device)
        self.state = torch.zeros((n, self._state_ints()), dtype=torch.int32, device=dev)
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
