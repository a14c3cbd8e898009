"""Batched MPC baseline policies (the reference's ``gym_anm/agents``)."""
from .mpc import (MPCAgent, MPCAgentConstant, MPCAgentExpected, MPCAgentPerfect, MPCAgentPerfectChain,  # noqa: F401
                  MPCAgentPerfectStream)
