"""Radial profiles of objects on maps (the reference's ``astrild.profiles``)."""
