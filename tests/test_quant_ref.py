"""CPU: tests/quant_ref.py's E4M3 rounding against torch's own cast."""
import numpy as np

import quant_ref


def test_e4m3_rounding_equals_torchs_cast_on_every_finite_bf16_below_256():
    import torch

    bits = np.arange(1 << 16, dtype=np.uint32) << 16
    v = bits.view(np.float32)
    v = v[np.isfinite(v) & (np.abs(v) < 256)]
    assert v.size > 34000 and np.any(v == 0) and np.any((v != 0) & (np.abs(v) < 2.0 ** -9))
    want = torch.from_numpy(v).to(torch.float8_e4m3fn).to(torch.float32).numpy()
    got = quant_ref.e4m3(v.astype(np.float64)).astype(np.float32)
    assert got.tobytes() == want.tobytes()  # signs of zeros included
