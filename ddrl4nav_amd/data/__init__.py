from ddrl4nav_amd.data.experience import Experience
from ddrl4nav_amd.data.ring import PinnedRing
from ddrl4nav_amd.data.easybytes import EasyBytes
from ddrl4nav_amd.data.frame_planes import FramePlanes
from ddrl4nav_amd.data.demo_pool import DemoPool

__all__ = ["Experience", "PinnedRing", "EasyBytes", "FramePlanes", "DemoPool"]
