"""CREPE pitch network (torchcrepe's `Crepe`, the model behind the reference's `F0_Extractor('crepe')`) executed by libddsp_amd.

`Crepe(model)` has exactly torchcrepe's state-dict keys and shapes for 'full' and 'tiny' (`conv{i}.weight` (Cout, Cin, k, 1),
`conv{i}.bias`, `conv{i}_BN.{weight,bias,running_mean,running_var,num_batches_tracked}`, `classifier.{weight,bias}`), so
torchcrepe's `assets/full.pth` loads with `strict=True`.  `activations(audio16 (B,T))` runs framing, network and sigmoid on the
device only (a CPU tensor raises RuntimeError).  Inference only: nothing here records gradients.

The library keeps its prepared copies of the weights (repacked convolutions, batch norms folded into a scale and a shift)
while the parameters' values stand, as `hipddsp.WeightTable` describes: a write that torch does not count (into `p.data`)
needs `rebind()`.
"""
import torch
from torch import nn

import hipddsp

SAMPLE_RATE = 16000
HOP = 80           # samples at 16 kHz between frames (the reference's torchcrepe.predict(..., 16000, 80, ...))
PITCH_BINS = 360
WIDTHS = {"full": (1024, 128, 128, 128, 256, 512), "tiny": (128, 16, 16, 16, 32, 64)}
KERNELS = (512, 64, 64, 64, 64, 64)
BN_EPS = 0.0010000000474974513
CENTS_OFFSET = 1997.3794084376191


def n_frames(T16, hop=HOP):
    """CREPE frames of T16 samples at 16 kHz with pad=True (`ddsp_crepe_frames`): 1 + T16 // hop."""
    return hipddsp.crepe_frames(T16, hop)


class _Conv(nn.Module):
    def __init__(self, c_in, c_out, k):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(c_out, c_in, k, 1))
        self.bias = nn.Parameter(torch.zeros(c_out))


class _BatchNorm(nn.Module):
    """`nn.BatchNorm2d(c, eps=0.0010000000474974513, momentum=0.0)` in eval mode: its five state-dict entries."""

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Linear(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n_out, n_in))
        self.bias = nn.Parameter(torch.zeros(n_out))


class Crepe(nn.Module):
    def __init__(self, model="full"):
        super().__init__()
        if model not in WIDTHS:
            raise ValueError(f"Crepe: model must be 'full' or 'tiny', got {model!r}")
        self.model = model
        widths = WIDTHS[model]
        c_in = (1,) + widths[:-1]
        for i in range(6):
            setattr(self, f"conv{i + 1}", _Conv(c_in[i], widths[i], KERNELS[i]))
            setattr(self, f"conv{i + 1}_BN", _BatchNorm(widths[i]))
        self.classifier = _Linear(4 * widths[5], PITCH_BINS)
        self._table = hipddsp.WeightTable(hipddsp.CrepeWeights, Crepe._named_tensors, "Crepe",
                                          width=(hipddsp._int * 6)(*widths))

    def _named_tensors(self):
        """(CrepeWeights field, tensor) in the order of `ddsp_crepe_weights`."""
        out = []
        for field, attr in (("conv{}_w", "weight"), ("conv{}_b", "bias")):
            out += [(field.format(i), getattr(getattr(self, f"conv{i}"), attr)) for i in range(1, 7)]
        for field, attr in (("bn{}_w", "weight"), ("bn{}_b", "bias"), ("bn{}_mean", "running_mean"),
                            ("bn{}_var", "running_var")):
            out += [(field.format(i), getattr(getattr(self, f"conv{i}_BN"), attr)) for i in range(1, 7)]
        return out + [("cls_w", self.classifier.weight), ("cls_b", self.classifier.bias)]

    def rebind(self):
        """Forget the weight struct and have the library re-prepare the weights: after a submodule was replaced, or after a
        write `_version` does not count (`hipddsp.WeightTable`)."""
        self._table.invalidate()

    def _weights_struct(self):
        return self._table.struct(self)[0]

    @torch.no_grad()
    def activations(self, audio16, hop=HOP, n_samples=None, counts_dev=None):
        """:: (B, T) 16 kHz -> sigmoid activations (B, 1 + T // hop, 360) of torchcrepe.infer over torchcrepe.preprocess's
        frames (pad=True).
        `n_samples` (a sequence of B ints or a CPU integer tensor (B,), each giving at least 3 frames): a RAGGED batch.  A
        frame depends on its own 1024 samples only, so the network runs over the rows' own 1 + n_samples[b] // hop frames
        and over no padding; row b is what the call returns for audio16[b:b+1, :n_samples[b]] and exactly 0 after its
        frames.  A bad count raises ValueError before anything is launched.  (`counts_dev`: `Context.crepe_activations`.)"""
        if audio16.dim() != 2:
            raise ValueError("Crepe.activations: audio must be (B, T)")
        if n_samples is not None:
            n_samples = hipddsp.check_crepe_n_samples(n_samples, audio16.shape[0], audio16.shape[1], hop)
        if not audio16.is_cuda:
            raise RuntimeError("Crepe runs on a HIP device only (no CPU fallback)")
        x = audio16.contiguous().float()
        return hipddsp.context_for(x.device).crepe_activations(self._weights_struct(), x, hop, n_samples, counts_dev)

    def forward(self, audio16):
        return self.activations(audio16)


def frequency_to_bin(f, ceil=False):
    """torchcrepe.convert.frequency_to_bins in fp32 (the arithmetic of `torch.tensor(f)`): floor (or ceil) of
    (1200 log2(f / 10) - 1997.3794084376191) / 20."""
    t = torch.tensor(f, dtype=torch.float32)
    x = (1200 * torch.log2(t / 10.) - CENTS_OFFSET) / 20
    return int(torch.ceil(x) if ceil else torch.floor(x))


def bin_to_frequency(b):
    """Bin (tensor of ints) -> Hz without dither: 10 * 2^((20 b + 1997.3794084376191) / 1200) in fp32."""
    cents = 20 * torch.as_tensor(b) + CENTS_OFFSET
    return 10 * 2 ** (cents.float() / 1200)
