"""What the synthetic packed models (packed_resnet, packed_mobilenet, packed_vit: tests and tools/bench_*_forward.py) are
built from: the host-side tpack, the state_dict entries of a random conv and of the CNNs' fc, and the calibration skeleton.
Every function draws from `rng` in a fixed order with fixed arguments: the synthetic models are what the README's forward
figures were measured on, and tests/test_synthetic_digest_cpu.py pins their bytes."""
import numpy as np
import torch


def pack_codes(q, n_bits, signed):
    """tpack on the host: integer codes -> the little-endian b-bit stream (stored value q + 2^(b-1) when signed)."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    stored = (q + ((1 << (n_bits - 1)) if signed else 0)).astype(np.uint64)
    if n_bits == 8:
        return stored.astype(np.uint8)
    bits = ((stored[:, None] >> np.arange(n_bits, dtype=np.uint64)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def _quantizer_entries(qmin, qmax):
    return {"a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
            "a_quantizer.zero": torch.tensor([0.0], dtype=torch.float32),
            "a_quantizer.qmin": torch.tensor(float(qmin)), "a_quantizer.qmax": torch.tensor(float(qmax))}


def conv_entries(rng, IC, OC, K, w_bits, a_bits, a_signed, gain, groups=1):
    """A conv's state_dict entries: random b-bit weights, He-scaled by `gain`, a folded bias, the quantiser at scale 1."""
    lim = (1 << (w_bits - 1)) - 1
    IC //= groups                  # the input channels a weight sees: pack() stores w_des [b, s, OC, IC / groups, KH, KW]
    q = rng.randint(-lim, lim + 1, size=(OC, IC, K, K))
    std_q = np.sqrt(((2 * lim + 1) ** 2 - 1) / 12.0)
    ws = gain * np.sqrt(2.0 / (IC * K * K)) / std_q * rng.uniform(0.8, 1.2, size=OC)     # He-scaled
    qmin, qmax = (-(1 << (a_bits - 1)), (1 << (a_bits - 1)) - 1) if a_signed else (0, (1 << a_bits) - 1)
    return {"weight": torch.from_numpy(pack_codes(q, w_bits, True)),
            "w_des": torch.tensor([w_bits, 1, OC, IC, K, K], dtype=torch.int32),
            "w_scale": torch.from_numpy(ws.astype(np.float32).reshape(OC, 1, 1, 1)),
            "w_zero": torch.zeros((OC, 1, 1, 1), dtype=torch.float32),
            "bias": torch.from_numpy(rng.normal(0, 0.05, size=OC).astype(np.float32)),        # the folded BatchNorm's shift
            **_quantizer_entries(qmin, qmax)}


def fc_entries(rng, num_classes, K, w_bits, a_bits):
    """The CNNs' classifier behind the pooled post-ReLU features: an unsigned quantiser."""
    lim = (1 << (w_bits - 1)) - 1
    q = rng.randint(-lim, lim + 1, size=(num_classes, K))
    ws = np.sqrt(1.0 / K) / lim * rng.uniform(0.8, 1.2, size=(num_classes, 1))
    return {"weight": torch.from_numpy(pack_codes(q, w_bits, True)),
            "w_des": torch.tensor([w_bits, 1, num_classes, K], dtype=torch.int32),
            "w_scale": torch.from_numpy(ws.astype(np.float32)),
            "w_zero": torch.zeros((num_classes, 1), dtype=torch.float32),
            "bias": torch.from_numpy(rng.normal(0, 0.05, size=num_classes).astype(np.float32)),
            **_quantizer_entries(0, (1 << a_bits) - 1)}


def bn_entries(rng, C):
    """An unfolded BatchNorm2d's state_dict entries (the pre-activation families keep the BatchNorms in front of a block's
    first conv): gamma around 1, small beta and running mean, running variance around 1."""
    return {"weight": torch.from_numpy(rng.uniform(0.5, 1.5, size=C).astype(np.float32)),
            "bias": torch.from_numpy(rng.normal(0, 0.1, size=C).astype(np.float32)),
            "running_mean": torch.from_numpy(rng.normal(0, 0.1, size=C).astype(np.float32)),
            "running_var": torch.from_numpy(rng.uniform(0.5, 1.5, size=C).astype(np.float32)),
            "num_batches_tracked": torch.tensor(0, dtype=torch.int64)}


def put(sd, prefix, entries):
    for k, v in entries.items():
        sd[prefix + "." + k] = v


def calibration_images(images, batch, size, seed):
    """device -> `images`, or when None the seeded calibration batch of a synthetic model built with `seed`."""
    def draw(device):
        if images is not None:
            return images
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        return torch.randn(batch, 3, size, size, generator=g).to(device)
    return draw


def calibrated(sd, device, build, images, quantisers):
    """`sd` on `device` with the activation quantisers of build(sd).calibrate(images(device)) written back (the batch is
    drawn once the state_dict is on the device); quantisers(model) is the model's {key: tensor} of them."""
    sd = {k: v.to(device) for k, v in sd.items()}
    model = build(sd).calibrate(images(device))
    for k, v in quantisers(model).items():
        sd[k] = v.detach().clone()
    return sd
