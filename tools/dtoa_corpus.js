'use strict'
// Number-to-string corpus for ygm_dtoa.hpp (test tooling): what V8's Number.prototype.toString gives for a list of
// doubles -- the edges at which the shortest-digits search or the layout can go wrong, then seeded random bit patterns
// (the PRNG is mulberry32 below; NaN and the infinities left out) -- and for float32 values widened to doubles, as the
// float32 tag of an Any is read.
//   doubles   [[16 hex digits of the double, most significant byte first, String(x)], ...]
//   floats    [[8 hex digits of the float32, String(Math.fround value)], ...]
//   node tools/dtoa_corpus.js <out.json.gz>
const fs = require('fs')
const zlib = require('zlib')

const RANDOM = 4000
const RANDOM_F32 = 500

function mulberry32 (a) {
  return () => {
    a |= 0; a = a + 0x6D2B79F5 | 0
    let t = Math.imul(a ^ a >>> 15, 1 | a)
    t = t + Math.imul(t ^ t >>> 7, 61 | t) ^ t
    return ((t ^ t >>> 14) >>> 0) / 4294967296
  }
}
const buf = Buffer.alloc(8)
const hexOf = x => { buf.writeDoubleBE(x, 0); return buf.toString('hex') }
const ofBits = (hi, lo) => { buf.writeUInt32BE(hi >>> 0, 0); buf.writeUInt32BE(lo >>> 0, 4); return buf.readDoubleBE(0) }
const prev = x => { buf.writeDoubleBE(x, 0); const v = buf.readBigUInt64BE(0) - 1n; buf.writeBigUInt64BE(v, 0); return buf.readDoubleBE(0) }   // (x > 0)

function edgeDoubles () {
  const xs = [5e-324, 2.2250738585072014e-308, prev(2.2250738585072014e-308), 1.7976931348623157e+308,
    0.1, 0.3, 0.1 + 0.2, 4.35, 0.000001, 1e-7, 1.5e-7, 123456.789,
    1e21, 999999999999999900000, 1e22, 1e23, 9.999999999999999e22,
    Math.pow(2, 53), Math.pow(2, 53) + 2, Math.pow(2, 60), Math.pow(2, 63), Math.pow(2, 64),
    Math.pow(2, -1022), -0, 0, -1.5, 100.25, 0.5, 1 / 3,
    // the layout's borders: n = 21 / 22, n = -5 / -6, k = n, the longest strings
    123456789012345680000, 1234567890123456800000, 0.000001234, 1.234e-7, -0.0000027410441684333906, -1.7976931348623157e+308,
    1, 10, 100, 1e15, 1e16, 1e17, 12345678.9, 0.001, 1.5, -42, 9007199254740993, 4294967296, 1700000000000,
    Math.fround(0.1), 16777216, Math.fround(3.4028234663852886e+38)]
  for (let k = -1074; k <= 1023; k += 19) { const p = Math.pow(2, k); xs.push(p); if (k > -1074) xs.push(prev(p)) }   // a power of two and its (nearer) lower neighbour
  return xs
}
function edgeFloats () {
  const f = Buffer.alloc(4)
  const bits = x => { f.writeFloatBE(x, 0); return f.readUInt32BE(0) }
  return [bits(0.1), bits(16777217), bits(3.4028234663852886e+38), bits(1.5), bits(-0), 1, 0x007FFFFF, 0x00800000, 0x00000400, bits(-1e-40), bits(1 / 3), bits(1e10)]
}

if (require.main === module) {
  const rnd = mulberry32(20251)
  const doubles = edgeDoubles().map(x => [hexOf(x), String(x)])
  while (doubles.length < edgeDoubles().length + RANDOM) {
    const x = ofBits(rnd() * 4294967296, rnd() * 4294967296)
    if (Number.isFinite(x)) doubles.push([hexOf(x), String(x)])
  }
  const f = Buffer.alloc(4)
  const floats = []
  const pushF = u => { f.writeUInt32BE(u >>> 0, 0); const x = f.readFloatBE(0); if (Number.isFinite(x)) floats.push([f.toString('hex'), String(x)]) }
  edgeFloats().forEach(pushF)
  while (floats.length < edgeFloats().length + RANDOM_F32) pushF(rnd() * 4294967296)
  const doc = { source: "tools/dtoa_corpus.js (V8's Number.prototype.toString): node tools/dtoa_corpus.js tests/golden/dtoa_v8.json.gz", doubles, floats }
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  console.log(JSON.stringify({ doubles: doubles.length, floats: floats.length }))
}

module.exports = { edgeDoubles, edgeFloats }
