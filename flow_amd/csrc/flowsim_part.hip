// flowsim_part.hip -- one object of libflowsim.so per (precision, lanes per replica): compiled by flow_amd/build.py with
//   -DFS_PART_T=float|double  and  -DFS_PART_SEG=8|16|32|64  (one wave carries 64 / SEG replicas)
//                              or  -DFS_PART_WIDE=2|4         (one workgroup of 2 / 4 waves per replica)
//                              or  -DFS_PART_QUEUE=1          (the queue-order kernels of the open networks, float32)
//                              or  -DFS_PART_LEARN=1          (the PPO update's kernels and their launchers, float32)
// so that the step kernels of the pairs compile in parallel and an edit to one kernel family rebuilds few objects.
#include "flowsim_launch.h"
#include "flowsim_learn.h"       // (FS_PART_LEARN: defines k_ppo_eval, k_gae, k_ppo_grad, k_adv_stats, k_adv_finish, k_adam and their fsim::launch_*)
#include "flowsim_es.h"          // (FS_PART_LEARN: defines k_es_perturb, k_es_fitness, k_es_weights, k_es_grad and their fsim::launch_*)

namespace fsim {
#if defined(FS_PART_LEARN)
#elif defined(FS_PART_QUEUE)
template int Sim<FS_PART_T>::launch_queue(const StepArgs&);
template int Sim<FS_PART_T>::launch_dropq(const StepArgs&);
template int Sim<FS_PART_T>::launch_policy_queue(const fs::PolicyView&, int, int, float*, float*, float*, float*, uint8_t*);
template int Sim<FS_PART_T>::launch_policy_act_vec(const fs::PolicyView&, const float*, float*, float*);
template int Sim<FS_PART_T>::launch_policy_act_wide(const fs::PolicyView&, const float*, float*, float*);
#elif defined(FS_PART_WIDE)
template int Sim<FS_PART_T>::launch_wide<FS_PART_WIDE>(const StepArgs&);
#elif defined(FS_PART_SEG)
template int Sim<FS_PART_T>::launch_open<FS_PART_SEG>(const StepArgs&);
template int Sim<FS_PART_T>::launch_ml<FS_PART_SEG>(const StepArgs&);
template int Sim<FS_PART_T>::launch_ring<FS_PART_SEG>(const StepArgs&);
template int Sim<FS_PART_T>::launch_pair<FS_PART_SEG>(const StepArgs&);
template int Sim<FS_PART_T>::launch_idm<FS_PART_SEG>(const StepArgs&);
template int Sim<FS_PART_T>::launch_k_steps<FS_PART_SEG>(const StepArgs&);
#if FS_PART_SEG == 16
template int Sim<FS_PART_T>::launch_loop(const StepArgs&);
template int Sim<FS_PART_T>::launch_policy_loop16(const fs::PolicyView&, int, int, float*, float*, float*, float*, uint8_t*);
template int Sim<FS_PART_T>::launch_policy_act_row16(const fs::PolicyView&, const float*, float*, float*);
template int Sim<FS_PART_T>::launch_policy_pair16(const fs::PolicyView&, const fs::PolicyView&, float, int, int, const float*,
                                                  float*, float*, float*, float*, float*, uint8_t*);
#endif
#if FS_PART_SEG == 32
template int Sim<FS_PART_T>::launch_policy_act(const fs::PolicyView&, int, const float*, float*, float*);
template int Sim<FS_PART_T>::launch_policy_row16(const fs::PolicyView&, int, int, float*, float*, float*, float*, uint8_t*);
#endif
#if FS_PART_SEG == 64
template int Sim<FS_PART_T>::launch_obs_mixed(const StepArgs&);     // (one object: the kernel does not depend on the width)
#endif
#else
#error "flowsim_part.hip: define FS_PART_T and FS_PART_SEG, FS_PART_WIDE, FS_PART_QUEUE or FS_PART_LEARN"
#endif
}  // namespace fsim
