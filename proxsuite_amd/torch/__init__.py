"""`proxsuite.torch` of the reference: the QPLayer forward on the MI355X batch solver."""
from .qplayer import QPFunction, solution_jacobians

__all__ = ["QPFunction", "solution_jacobians"]
