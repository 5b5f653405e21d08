// The 36 temporaries of the hand-written loops of k_pcg_pipe (pcg_pipe_stream.hip.h, pcg_pipe_onchip.hip.h) by name: FBV_<n> is the register the
// loops call v<n>, FBV_<n>_<m> the range v[n:m].  Two sets.  The default one is v120..v155 itself: every instantiation that was built before the
// register slots (pcg_pipe_regs.hip.h) keeps its code register for register.  With FBP_TEMPS_LOW defined the same names are v64..v99 -- the
// compiler then packs the solver's state around them into 138 registers instead of 168, and the 30 it leaves hold matrix values
// (pcg_pipe_regs.hip.h).  No include guard: including this file again
// renames the temporaries for the text that follows.
// clang-format off
#ifdef FBV_120
#undef FBV_120
#undef FBV_121
#undef FBV_122
#undef FBV_123
#undef FBV_124
#undef FBV_125
#undef FBV_126
#undef FBV_127
#undef FBV_128
#undef FBV_129
#undef FBV_130
#undef FBV_131
#undef FBV_132
#undef FBV_133
#undef FBV_134
#undef FBV_135
#undef FBV_136
#undef FBV_137
#undef FBV_138
#undef FBV_139
#undef FBV_140
#undef FBV_141
#undef FBV_142
#undef FBV_143
#undef FBV_144
#undef FBV_145
#undef FBV_146
#undef FBV_147
#undef FBV_148
#undef FBV_149
#undef FBV_150
#undef FBV_151
#undef FBV_152
#undef FBV_153
#undef FBV_154
#undef FBV_155
#undef FBV_120_121
#undef FBV_122_123
#undef FBV_124_125
#undef FBV_124_127
#undef FBV_126_127
#undef FBV_128_129
#undef FBV_130_131
#undef FBV_130_133
#undef FBV_132_133
#undef FBV_134_135
#undef FBV_136_137
#undef FBV_138_139
#undef FBV_140_141
#undef FBV_142_143
#undef FBV_144_145
#undef FBV_146_147
#undef FBV_152_153
#endif
#ifdef FBP_TEMPS_LOW
#define FBV_120 "v64"
#define FBV_121 "v65"
#define FBV_122 "v66"
#define FBV_123 "v67"
#define FBV_124 "v68"
#define FBV_125 "v69"
#define FBV_126 "v70"
#define FBV_127 "v71"
#define FBV_128 "v72"
#define FBV_129 "v73"
#define FBV_130 "v74"
#define FBV_131 "v75"
#define FBV_132 "v76"
#define FBV_133 "v77"
#define FBV_134 "v78"
#define FBV_135 "v79"
#define FBV_136 "v80"
#define FBV_137 "v81"
#define FBV_138 "v82"
#define FBV_139 "v83"
#define FBV_140 "v84"
#define FBV_141 "v85"
#define FBV_142 "v86"
#define FBV_143 "v87"
#define FBV_144 "v88"
#define FBV_145 "v89"
#define FBV_146 "v90"
#define FBV_147 "v91"
#define FBV_148 "v92"
#define FBV_149 "v93"
#define FBV_150 "v94"
#define FBV_151 "v95"
#define FBV_152 "v96"
#define FBV_153 "v97"
#define FBV_154 "v98"
#define FBV_155 "v99"
#define FBV_120_121 "v[64:65]"
#define FBV_122_123 "v[66:67]"
#define FBV_124_125 "v[68:69]"
#define FBV_124_127 "v[68:71]"
#define FBV_126_127 "v[70:71]"
#define FBV_128_129 "v[72:73]"
#define FBV_130_131 "v[74:75]"
#define FBV_130_133 "v[74:77]"
#define FBV_132_133 "v[76:77]"
#define FBV_134_135 "v[78:79]"
#define FBV_136_137 "v[80:81]"
#define FBV_138_139 "v[82:83]"
#define FBV_140_141 "v[84:85]"
#define FBV_142_143 "v[86:87]"
#define FBV_144_145 "v[88:89]"
#define FBV_146_147 "v[90:91]"
#define FBV_152_153 "v[96:97]"
#else
#define FBV_120 "v120"
#define FBV_121 "v121"
#define FBV_122 "v122"
#define FBV_123 "v123"
#define FBV_124 "v124"
#define FBV_125 "v125"
#define FBV_126 "v126"
#define FBV_127 "v127"
#define FBV_128 "v128"
#define FBV_129 "v129"
#define FBV_130 "v130"
#define FBV_131 "v131"
#define FBV_132 "v132"
#define FBV_133 "v133"
#define FBV_134 "v134"
#define FBV_135 "v135"
#define FBV_136 "v136"
#define FBV_137 "v137"
#define FBV_138 "v138"
#define FBV_139 "v139"
#define FBV_140 "v140"
#define FBV_141 "v141"
#define FBV_142 "v142"
#define FBV_143 "v143"
#define FBV_144 "v144"
#define FBV_145 "v145"
#define FBV_146 "v146"
#define FBV_147 "v147"
#define FBV_148 "v148"
#define FBV_149 "v149"
#define FBV_150 "v150"
#define FBV_151 "v151"
#define FBV_152 "v152"
#define FBV_153 "v153"
#define FBV_154 "v154"
#define FBV_155 "v155"
#define FBV_120_121 "v[120:121]"
#define FBV_122_123 "v[122:123]"
#define FBV_124_125 "v[124:125]"
#define FBV_124_127 "v[124:127]"
#define FBV_126_127 "v[126:127]"
#define FBV_128_129 "v[128:129]"
#define FBV_130_131 "v[130:131]"
#define FBV_130_133 "v[130:133]"
#define FBV_132_133 "v[132:133]"
#define FBV_134_135 "v[134:135]"
#define FBV_136_137 "v[136:137]"
#define FBV_138_139 "v[138:139]"
#define FBV_140_141 "v[140:141]"
#define FBV_142_143 "v[142:143]"
#define FBV_144_145 "v[144:145]"
#define FBV_146_147 "v[146:147]"
#define FBV_152_153 "v[152:153]"
#endif
// clang-format on
