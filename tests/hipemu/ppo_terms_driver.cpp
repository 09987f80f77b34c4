// TEST INFRASTRUCTURE ONLY: seqdex_amd/csrc/sdxp_ppo_terms.h (the product's header, compiled by g++ for the CPU) as plain loops over the
// rows and actions of one minibatch, and its step rules, for tests/test_ppo_terms_host.py.
#include <hip/hip_runtime.h>
#include <string.h>

#include "sdxp_ppo_terms.h"

// mu / act / omu / osg / dmu: [M][A]; the per-row inputs and v0 (critic) / v1 (central value): [M]; rows: [M][8] = surrogate, critic loss,
// central-value loss, bound loss, KL, entropy, d loss / d v0, d loss / d v1; dls: [A] = d loss / d logstd with the entropy term
extern "C" void ppo_terms_minibatch(int M, int A, float e_clip, float critic_coef, float bounds_coef, float entropy_coef, int clip_value,
                                    const float* logstd, const float* mu, const float* act, const float* omu, const float* osg, const float* adv,
                                    const float* old_nlp, const float* ret, const float* old_v, const float* v0, const float* v1, float* rows,
                                    float* dmu, float* dls) {
  SdxpDev D;
  memset(&D, 0, sizeof(D));
  D.e_clip = e_clip; D.critic_coef = critic_coef; D.bounds_coef = bounds_coef; D.entropy_coef = entropy_coef; D.clip_value = clip_value;
  const float invM = 1.0f / (float)M;
  for (int a = 0; a < A; ++a) dls[a] = 0.0f;
  for (int s = 0; s < M; ++s) {
    float nlp = 0.0f, kl = 0.0f, bl = 0.0f, ent = 0.0f, z[64];
    for (int a = 0; a < A; ++a) {
      const PpoActionTerms t = ppo_action_terms(logstd[a], expf(logstd[a]), mu[s * A + a], act[s * A + a], omu[s * A + a], osg[s * A + a]);
      nlp += t.nlp; kl += t.kl; bl += t.bl; ent += t.ent; z[a] = t.z;
    }
    const PpoRowTerms r = ppo_row_terms(D, adv[s], old_nlp[s], ppo_neglogp(nlp, A), ret[s], old_v[s], v0[s], v1[s], invM);
    const float out[8] = {r.a_loss, r.closs[0], r.closs[1], bl, kl, ent, r.dv[0], r.dv[1]};
    memcpy(rows + 8 * s, out, sizeof(out));
    for (int a = 0; a < A; ++a) {
      const PpoActionGrad g = ppo_action_grad(r.gnlp, z[a], expf(logstd[a]), mu[s * A + a], bounds_coef, invM);
      dmu[s * A + a] = g.dmu;
      dls[a] += g.dls;
    }
  }
  for (int a = 0; a < A; ++a) dls[a] = ppo_dlogstd(dls[a], entropy_coef);
}
extern "C" float ppo_terms_lr(float lr, float kl, float kl_threshold) { return ppo_adaptive_lr(lr, kl, kl_threshold); }
extern "C" float ppo_terms_clip_scale(int truncate_grads, float grad_norm, float norm) {
  SdxpDev D;
  memset(&D, 0, sizeof(D));
  D.truncate_grads = truncate_grads; D.grad_norm = grad_norm;
  return ppo_clip_scale(D, norm);
}
extern "C" void ppo_terms_adam_bias(int t0, int n, float* bc1, float* bc2) {
  for (int i = 0; i < n; ++i) { const PpoBias b = ppo_adam_bias(t0 + i); bc1[i] = b.bc1; bc2[i] = b.bc2; }
}
