"""DemoPool: a ring of demonstrations on the device -- observation components and the expert's labels, a row per env and step -- that a
device env renders into and an expert writes into directly.  Nothing is copied on the way in: ``rows(t)``
hands out views, the env's step takes the component views as ``obs_out`` and the expert the label view as ``labels_out``."""
import numpy as np
import torch


def slot_of(t, n_slots):
    """The slot (a block of n_envs rows) step t of the pool's life writes: t mod n_slots."""
    return int(t) % int(n_slots)


def labelled_rows(cursor, pending, n_slots, n_envs):
    """int64 row indices that hold an observation WITH its label after `cursor` row sets were opened, the last of them still waiting for
    its label when `pending`: rows of slots that were never opened, and the pending slot (which, once the ring is full, has overwritten
    the oldest labelled rows), are left out."""
    opened = min(int(cursor), int(n_slots))
    slots = np.arange(opened, dtype=np.int64)
    if pending:
        slots = slots[slots != slot_of(cursor - 1, n_slots)]
    return (slots[:, None] * int(n_envs) + np.arange(int(n_envs), dtype=np.int64)[None, :]).reshape(-1)


def same_device(a, b):
    """True when two torch devices name the same card ("cuda" is the current one)."""
    a, b = torch.device(a), torch.device(b)
    index = lambda d: d.index if d.index is not None or d.type != "cuda" else torch.cuda.current_device()
    return a.type == b.type and index(a) == index(b)


class DemoPool:
    def __init__(self, state_shapes, action_dim, capacity, device=None, n_envs=1):
        """state_shapes: the shapes of the observation components (DeviceNavEnv.state_shapes), held as fp32 [capacity, ...]; labels
        fp32 [capacity, action_dim].  The write cursor advances n_envs rows per step; capacity is a multiple of n_envs, and a full pool
        overwrites its oldest rows."""
        self.action_dim, self.capacity, self.n_envs = int(action_dim), int(capacity), int(n_envs)
        if self.n_envs < 1 or self.action_dim < 1:
            raise ValueError("n_envs and action_dim must be at least 1, got %d and %d" % (self.n_envs, self.action_dim))
        if self.capacity < 2 * self.n_envs or self.capacity % self.n_envs:
            raise ValueError("capacity must be a multiple of n_envs = %d and hold at least two steps, got %d" % (self.n_envs, self.capacity))
        shapes = [tuple(int(d) for d in s) for s in state_shapes]
        if not shapes or any(len(s) < 1 or min(s) < 1 for s in shapes):
            raise ValueError("state_shapes must name at least one component with positive dimensions, got %r" % (state_shapes,))
        self.device = torch.device("cuda:%d" % torch.cuda.current_device() if device is None or str(device) == "cuda" else device)
        self.n_slots = self.capacity // self.n_envs
        f32 = dict(dtype=torch.float32, device=self.device)
        self.components = [torch.zeros((self.capacity,) + s, **f32) for s in shapes]
        self.labels = torch.zeros((self.capacity, self.action_dim), **f32)
        self.cursor = 0          # row sets opened so far: set t lives in slot t mod n_slots
        self.pending = False     # the last opened set holds an observation that still waits for its label

    def rows(self, t):
        """(component views, label view) of row set t: [n_envs, ...] each, views of the pool's own tensors."""
        lo = slot_of(t, self.n_slots) * self.n_envs
        return [c[lo:lo + self.n_envs] for c in self.components], self.labels[lo:lo + self.n_envs]

    def open(self):
        """Opens the next row set for an observation and returns its index t; its label follows with close_label()."""
        if self.pending:
            raise RuntimeError("the last row set still waits for its label")
        self.cursor += 1
        self.pending = True
        return self.cursor - 1

    def close_label(self):
        """The pending row set has its label."""
        if not self.pending:
            raise RuntimeError("no row set waits for a label")
        self.pending = False

    def put(self, components, labels):
        """Recorded demonstrations: copies whole row sets (a multiple of n_envs rows: components [m, ...], labels [m, action_dim], host
        or device) in at the cursor, each with its label."""
        labels = torch.as_tensor(labels, dtype=torch.float32).reshape(-1, self.action_dim)
        m = labels.shape[0]
        if m < self.n_envs or m % self.n_envs or len(components) != len(self.components):
            raise ValueError("put takes %d components of a multiple of %d rows, got %d of %d" % (len(self.components), self.n_envs,
                                                                                                   len(components), m))
        comps = [torch.as_tensor(c, dtype=torch.float32).reshape((m,) + tuple(mine.shape[1:])) for c, mine in zip(components, self.components)]
        for k in range(m // self.n_envs):
            dst, lab = self.rows(self.open())
            lo = k * self.n_envs
            for d, c in zip(dst, comps):
                d.copy_(c[lo:lo + self.n_envs])
            lab.copy_(labels[lo:lo + self.n_envs])
            self.close_label()

    def labelled_rows(self):
        """int64 indices of the rows that hold an observation with its label."""
        return labelled_rows(self.cursor, self.pending, self.n_slots, self.n_envs)

    def __len__(self):
        return len(self.labelled_rows())
