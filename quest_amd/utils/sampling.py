"""Device-side token sampling (EXTENSION; include/quest_hip.h, "Token sampling"): the parameters and the per-sequence state
of the sampling launch, kept in device memory so that a captured decode step can end with the token choice and feed the
next step without a host round trip.

The reference samples on the host: ``model.generate`` of transformers in its scripts, a temperature / top-p / top-k sampler
with a stop token in scripts/example_demo.py.  The filter order here is transformers' (temperature, top-k, top-p).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import torch

from .. import _kernels


@dataclass
class SamplingParams:
    """``temperature`` 0 = greedy (the first token by 16-bit key, ties to the lowest index); ``top_k`` <= 0 = no top-k;
    ``top_p`` >= 1 = no top-p; ``seed``: any 64-bit integer -- a sequence's tokens depend on (seed, position) only, not on
    the batch it is decoded in."""
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0


class Sampler:
    """The device arrays of ``n`` sequences' sampling: parameters, finished flags, eos ids, the token history
    (``[n, max_tokens]``) and the last tokens.  ``set_params`` writes into them in place: a decode graph captured over a
    sampler keeps serving after a change of parameters."""

    def __init__(self, n: int, vocab_size: int, device, max_tokens: int = 0,
                 eos_token_id: Union[None, int, Sequence[int]] = None, pad_id: Optional[int] = None):
        eos = [] if eos_token_id is None else [eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)
        if len(eos) > _kernels.SAMPLE_MAX_EOS:
            raise ValueError(f"at most {_kernels.SAMPLE_MAX_EOS} eos ids ({len(eos)} given)")
        if not 1 <= vocab_size <= _kernels.SAMPLE_MAX_VOCAB:
            raise ValueError(f"vocab_size {vocab_size}: the sampling launch serves 1 .. {_kernels.SAMPLE_MAX_VOCAB}")
        self.pad_id = int(pad_id if pad_id is not None else (eos[0] if eos else 0))
        for t in eos + [self.pad_id]:
            if not 0 <= t < vocab_size:
                raise ValueError(f"token id {t} outside the vocabulary of {vocab_size}")
        self.n, self.vocab_size, self.device = n, vocab_size, device
        with torch.inference_mode(False):  # ordinary tensors whatever mode the caller is in: only launches write them
            self.temperature = torch.zeros(n, dtype=torch.float32, device=device)
            self.top_k = torch.zeros(n, dtype=torch.int32, device=device)
            self.top_p = torch.ones(n, dtype=torch.float32, device=device)
            self.seed = torch.zeros(n, dtype=torch.int64, device=device)
            self.tokens = torch.zeros(n, dtype=torch.int32, device=device)
            self.kept = torch.zeros(n, dtype=torch.int32, device=device)
            self.finished = torch.zeros(n, dtype=torch.int32, device=device)
            self.eos_ids = torch.tensor(eos, dtype=torch.int32, device=device) if eos else None
            self.history = torch.zeros(n, max_tokens, dtype=torch.int32, device=device) if max_tokens > 0 else None
            self.history_len = torch.zeros(n, dtype=torch.int32, device=device) if max_tokens > 0 else None

    def set_params(self, seq: int, params: SamplingParams) -> None:
        seed = int(params.seed) & 0xFFFFFFFFFFFFFFFF
        with torch.inference_mode():
            self.temperature[seq] = float(params.temperature)
            self.top_k[seq] = int(params.top_k)
            self.top_p[seq] = float(params.top_p)
            self.seed[seq] = seed - (1 << 64) if seed >= 1 << 63 else seed  # the uint64's bits in an int64 tensor

    def reset(self) -> None:
        """Start a new request: no sequence finished, empty histories."""
        with torch.inference_mode():
            self.finished.zero_()
            if self.history_len is not None:
                self.history_len.zero_()

    def snapshot(self):
        return self.finished.clone(), None if self.history_len is None else self.history_len.clone()

    def restore(self, saved) -> None:
        with torch.inference_mode():
            self.finished.copy_(saved[0])
            if self.history_len is not None:
                self.history_len.copy_(saved[1])

    def sample(self, logits: torch.Tensor, *, states=None, positions=None, embed=None, next_input=None) -> torch.Tensor:
        """One launch: ``logits`` ``[n, vocab]`` -> ``self.tokens`` (int32 ``[n]``), the flags and the history; with
        ``embed`` / ``next_input`` also the next step's input rows.  Positions from ``states`` (``[n, 8]`` step states,
        as inside a captured step) or ``positions`` (int32 ``[n]``: the index each sampled token will occupy)."""
        _kernels.sample_tokens(logits, self.temperature, self.top_k, self.top_p, self.seed, self.tokens, states=states,
                               positions=positions, kept=self.kept, eos_ids=self.eos_ids, pad_id=self.pad_id,
                               finished=self.finished, history=self.history, history_len=self.history_len, embed=embed,
                               next_input=next_input)
        return self.tokens

    def all_finished(self) -> bool:
        """Reads the flags back (a device-to-host copy)."""
        return bool(self.finished.all().item())

    def sequences(self) -> List[torch.Tensor]:
        """Each sequence's generated tokens (int64, CPU), ending with its eos id when it reached one."""
        lens = self.history_len.cpu().tolist()
        hist = self.history.cpu()
        return [hist[i, :lens[i]].to(torch.int64) for i in range(self.n)]
