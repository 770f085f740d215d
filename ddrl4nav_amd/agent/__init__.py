from ddrl4nav_amd.agent.agent import Agents, gae_device
from ddrl4nav_amd.agent.rollout import DeviceRollout, StateRollout
from ddrl4nav_amd.agent.plane_rollout import PlaneRollout
from ddrl4nav_amd.agent.statistics import EpisodeReturns, NavStatus
from ddrl4nav_amd.agent.normalize import RunningNorm

__all__ = ["Agents", "gae_device", "DeviceRollout", "PlaneRollout", "StateRollout", "EpisodeReturns", "NavStatus", "RunningNorm"]
