"""Base agents: AgentBase, AgentPPO (on-policy, the residual agents' parent), AgentOffPolicy and AgentTD3
(interface of the reference's elegantrl/agent.py: AgentBase :15-124, AgentTD3 :276-394, AgentPPO :543-712; AgentSAC :397-478
is in agent_sac.py).  AgentOffPolicy is not in the reference: it is the host path that AgentTD3 and
AgentSAC share -- vectorised exploration into a VecReplayBuffer and `update_net` on a fused optimizer step (index tables, one
HIP graph per update) -- so that each agent keeps only its own arithmetic.

What differs from the reference, by design:
  * `explore_env` understands vectorised envs (`env.num_envs`): all N lanes advance in lock-step, the policy
    runs once per step on [N, D], and transitions go straight into a time-major `TrajectoryBuffer` in HBM.
    A one-instance env (the gym-style facade) still takes the reference's per-step loop.
  * the value pass and the rollout policy mean run on the fused f32-MFMA forward, GAE on the scan kernel
    (via the injected backend; the product backend is HIP-only).
  * loss scalars are accumulated on the device and read back once per `update_net`, not four `.item()` syncs
    per minibatch (agent.py:644-653).
  * under torch.distributed every optimizer step all-reduces ONE flat gradient buffer, and the buffer-global
    advantage normalisation (agent.py:707) all-reduces three moments.

The classes live in agent_base.py (AgentBase), agent_ppo.py (AgentPPO), agent_offpolicy.py (AgentOffPolicy, AgentTD3) and
agent_sac.py (AgentSAC); this module keeps the reference's name for them."""
from .agent_base import AgentBase  # noqa: F401
from .agent_offpolicy import AgentOffPolicy, AgentTD3  # noqa: F401
from .agent_ppo import AgentPPO  # noqa: F401
from .agent_sac import AgentSAC  # noqa: F401
