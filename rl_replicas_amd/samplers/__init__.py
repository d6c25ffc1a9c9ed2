from .sampler import Sampler
from .batch_sampler import BatchSampler
from .device_episodic_sampler import DeviceEpisodicSampler
from .device_sampler import DeviceSampler
from .device_replay_sampler import DeviceReplaySampler
from .vector_sampler import VectorSampler

__all__ = ["Sampler", "BatchSampler", "VectorSampler", "DeviceSampler",
           "DeviceEpisodicSampler", "DeviceReplaySampler"]
