"""Timestep samplers of the diffusion training loop (model/resample.py:6-48 of the reference): `sample(batch_size, device)` draws integer
steps with probability proportional to `weights()` and returns them with the importance weights 1 / (N p_t).  Only the uniform
sampler is built (train_latent.py:94 uses it)."""
import numpy as np
import torch


class UniformSampler:
    def __init__(self, num_timesteps):
        self._weights = np.ones([int(num_timesteps)])

    def weights(self):
        return self._weights

    def sample(self, batch_size, device):
        """-> (steps [batch_size] int64 in [0, num_timesteps), weights [batch_size] fp32), both on `device`."""
        w = self.weights()
        p = w / np.sum(w)
        indices_np = np.random.choice(len(p), size=(batch_size,), p=p)
        indices = torch.from_numpy(indices_np).long().to(device)
        weights = torch.from_numpy(1 / (len(p) * p[indices_np])).float().to(device)
        return indices, weights


def create_named_schedule_sampler(name, diffusion):
    if name == "uniform":
        return UniformSampler(diffusion.num_timesteps)
    raise NotImplementedError(f"unknown schedule sampler: {name} ('uniform' is built)")
