from ddrl4nav_amd.env.device_env import ENV_NAMES, DeviceEnv, make_device_env
from ddrl4nav_amd.env.device_nav_env import NAV_ENV_NAME, DeviceNavEnv

__all__ = ["DeviceEnv", "DeviceNavEnv", "make_device_env", "ENV_NAMES", "NAV_ENV_NAME"]
