"""What the explicit backwards of the HIP backbones (convnext.py, resnet.py) share."""

from __future__ import annotations

import torch


class ExplicitBackward:
    """Mixin of a backbone whose backward is an explicit kernel sequence: gradient buffers, readiness reports and the
    weight-gradient side stream.  The backbone's ``__init__`` sets ``grad_ready_hook``, ``_side`` ({}),
    ``comm_reserve_cus`` and ``comm_cu_mask``."""

    @staticmethod
    def _grad(p: torch.Tensor) -> torch.Tensor:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def _ready(self, params: list) -> None:
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(params)

    def _side_stream(self, device) -> torch.cuda.Stream:
        """The weight-gradient side stream; CU-masked (never on the CUs reserved for RCCL, training/cumask.py) when
        StepEngine asks for it (comm_reserve_cus > 0 and SV_COMM_CU_MASK=1)."""
        key = (device, self.comm_reserve_cus, self.comm_cu_mask)
        if key not in self._side:
            if self.comm_reserve_cus > 0 and self.comm_cu_mask:
                from ..training.cumask import reserved_stream

                self._side[key] = reserved_stream(device, self.comm_reserve_cus, "side")
            else:
                self._side[key] = torch.cuda.Stream(device=device)
        return self._side[key]
