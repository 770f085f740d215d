from ddrl4nav_amd.env.device_env import ENV_NAMES, DeviceEnv, make_device_env
from ddrl4nav_amd.env.device_nav_env import NAV_ENV_NAME, DeviceNavEnv
from ddrl4nav_amd.env.fleet_nav_env import FLEET_ENV_NAME, FleetNavEnv
from ddrl4nav_amd.env.nav_expert import NavExpert

__all__ = ["DeviceEnv", "DeviceNavEnv", "FleetNavEnv", "NavExpert", "make_device_env", "ENV_NAMES", "NAV_ENV_NAME", "FLEET_ENV_NAME"]
