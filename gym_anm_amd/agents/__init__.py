"""Batched MPC baseline policies (the reference's ``gym_anm/agents``)."""
from .mpc import MPCAgent, MPCAgentConstant, MPCAgentPerfect, MPCAgentPerfectChain, MPCAgentPerfectStream  # noqa: F401
