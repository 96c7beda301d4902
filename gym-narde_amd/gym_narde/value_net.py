"""The value network the scored afterstate calls evaluate on the device
(narde_afterstates_scored / narde_turn_afterstates_scored; DESIGN.md section
15): 198 -> H -> 1 over the Tesauro columns, TD-Gammon's shape.

ValueMLP is an ordinary torch module -- forward() is the dense evaluation,
the reference and the form autograd trains -- that also keeps the
feature-major copy of its first layer the kernels read.  The kernels read the
weights through pointers when they run, so after the weights change (an
optimiser step, load_state_dict) call pack() and the next launch -- or the
next replay of a captured graph -- sees them.
"""
import torch

from . import _lib

HIDDEN_MAX = 128  # NARDE_VALUE_HIDDEN_MAX
HIDDEN_ACTS = {"sigmoid": 0, "tanh": 1, "relu": 2}
OUT_ACTS = {"none": 0, "sigmoid": 1, "tanh": 2}
_ACT_FN = {"none": lambda x: x, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu}
_ACT_OF_MODULE = {torch.nn.Sigmoid: "sigmoid", torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu"}


class ValueMLP(torch.nn.Module):
    def __init__(self, hidden=80, hidden_act="sigmoid", out_act="sigmoid"):
        super().__init__()
        if not 1 <= int(hidden) <= HIDDEN_MAX:
            raise ValueError(f"hidden must be 1..{HIDDEN_MAX}")
        if hidden_act not in HIDDEN_ACTS:
            raise ValueError(f"hidden_act must be one of {tuple(HIDDEN_ACTS)}")
        if out_act not in OUT_ACTS:
            raise ValueError(f"out_act must be one of {tuple(OUT_ACTS)}")
        self.hidden, self.hidden_act, self.out_act = int(hidden), hidden_act, out_act
        self.l1 = torch.nn.Linear(198, self.hidden)
        self.l2 = torch.nn.Linear(self.hidden, 1)
        self._w1t = None  # (198, H) float32: l1.weight, feature-major

    @classmethod
    def from_sequential(cls, seq):
        """Adopt Sequential(Linear(198, H), act, Linear(H, 1)[, act]) -- the
        shape of examples/play_value_agent.py, so its checkpoints load."""
        mods = list(seq)
        if (len(mods) not in (3, 4) or not isinstance(mods[0], torch.nn.Linear) or mods[0].in_features != 198
                or not isinstance(mods[2], torch.nn.Linear) or mods[2].out_features != 1
                or mods[2].in_features != mods[0].out_features or type(mods[1]) not in _ACT_OF_MODULE):
            raise ValueError("expected Sequential(Linear(198, H), act, Linear(H, 1)[, act])")
        out = "none"
        if len(mods) == 4:
            if type(mods[3]) not in (torch.nn.Sigmoid, torch.nn.Tanh):
                raise ValueError("the output activation must be Sigmoid or Tanh")
            out = _ACT_OF_MODULE[type(mods[3])]
        net = cls(mods[0].out_features, _ACT_OF_MODULE[type(mods[1])], out)
        net.to(mods[0].weight.device)
        with torch.no_grad():
            net.l1.weight.copy_(mods[0].weight)
            net.l1.bias.copy_(mods[0].bias)
            net.l2.weight.copy_(mods[2].weight)
            net.l2.bias.copy_(mods[2].bias)
        return net

    def forward(self, feat):
        """(R,198) -> (R,): the dense evaluation."""
        h = _ACT_FN[self.hidden_act](self.l1(feat))
        return _ACT_FN[self.out_act](self.l2(h)).reshape(-1)

    def pack(self):
        """Refresh the feature-major copy of l1.weight: in place and
        stream-ordered, so a captured graph that holds struct()'s pointers
        reads the new weights at its next replay.  Returns self."""
        w = self.l1.weight
        if w.dtype != torch.float32 or not w.is_cuda:
            raise ValueError("the scored calls need float32 weights on a GPU device")
        with torch.no_grad():
            if self._w1t is None or self._w1t.device != w.device:
                self._w1t = torch.empty((198, self.hidden), dtype=torch.float32, device=w.device)
            self._w1t.copy_(w.t())
        return self

    def struct(self):
        """The ctypes narde_value_mlp over the live tensors (pack()ed on the
        first use; the module keeps them alive)."""
        if self._w1t is None or self._w1t.device != self.l1.weight.device:
            self.pack()
        for p in (self.l1.bias, self.l2.weight, self.l2.bias):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self._w1t.device:
                raise ValueError("the scored calls need contiguous float32 parameters on one device")
        return _lib.ValueMlp(self._w1t.data_ptr(), self.hidden, self.l1.bias.data_ptr(), self.l2.weight.data_ptr(),
                             self.l2.bias.data_ptr(), self.hidden, HIDDEN_ACTS[self.hidden_act],
                             OUT_ACTS[self.out_act])
