"""Radial profiles of objects on maps and of particles around haloes and voids (the reference's ``astrild.profiles``)."""
from .profile_3d import Profiles3D, radial_profiles

__all__ = ["Profiles3D", "radial_profiles"]
